"""CSCROIHeads on image batches (enable_image_batches): the head, the image-gradient passes, the backward and the eager
Trainer on 2-image batches made from the reference-generated fixture model_csc_r18dc5_tiny - its image, and the same image
(or a smaller crop of it) with its first 37 proposals and another label vector.  fp32, dropout off."""
import numpy as np
import pytest
import torch

import golden_util as G
from __graft_entry__ import load_package

pkg = load_package()
from drn_wsod_pytorch_amd._cabi import DrnError  # noqa: E402
from drn_wsod_pytorch_amd.engine import GraphedTrainStep, Trainer, build_optimizer  # noqa: E402

pytestmark = pytest.mark.gpu

NAME = "model_csc_r18dc5_tiny"


@pytest.fixture(autouse=True)
def _deterministic():
    """the atomic-free RoIPool backward: a map is then a function of its inputs alone (run to run, batch to single)"""
    pkg.set_deterministic(True)
    yield
    pkg.set_deterministic(False)


def _setup(crop=None):
    """-> (cfg, model, [image 0], [image 1]).  Image 1: the fixture image (crop = (H1, W1): its top-left crop, the boxes moved
    inside), its first 37 proposals, two classes image 0 does not have."""
    assert torch.cuda.is_available()
    ocfg = G.csc_case()
    d = G.load(NAME)
    cfg, model = G.drn_model(ocfg, int(d["seed"]), "cuda", 5, "fp32")
    heads = model.roi_heads
    heads.box_head.dropout_p = 0.0
    heads.tau, heads.iter = float(d["tau"]), int(d["iter0"])
    model.train()
    first = G.batch_from(d)[0]
    K = ocfg.num_classes
    other = [c for c in range(K) if c not in set(first["gt_classes"].tolist())]
    assert other, "the fixture labels every class: no other label vector"
    assert len(first["proposal_boxes"]) > 37
    boxes, image = first["proposal_boxes"][:37].clone(), first["image"]
    if crop is not None:
        H1, W1 = crop
        assert H1 < image.shape[1] and W1 < image.shape[2]
        image = image[:, :H1, :W1].clone()
        boxes[:, 0] = boxes[:, 0].clamp(0, W1 - 9)
        boxes[:, 1] = boxes[:, 1].clamp(0, H1 - 9)
        boxes[:, 2] = torch.maximum(boxes[:, 2].clamp(max=W1 - 1), boxes[:, 0] + 6)
        boxes[:, 3] = torch.maximum(boxes[:, 3].clamp(max=H1 - 1), boxes[:, 1] + 6)
    second = dict(first, image=image, proposal_boxes=boxes, objectness_logits=first["objectness_logits"][:37].clone(),
                  gt_classes=torch.tensor(other[:2], dtype=first["gt_classes"].dtype), gt_boxes=torch.zeros((len(other[:2]), 4)))
    return cfg, model, G.drn_inputs([first]), G.drn_inputs([second])


def _step(model, batch, it, tau, max_iter=None):
    """one forward + backward at a fixed head iteration -> (losses as float32 numpy, aux, gradients of the trainable weights)"""
    heads = model.roi_heads
    heads.iter, heads.tau = it, tau
    if max_iter is not None:
        heads.csc_max_iter = max_iter
    model.zero_grad()
    losses = model(batch)
    sum(losses.values()).backward()
    torch.cuda.synchronize()
    grads = {n: p.grad.detach().clone() for n, p in model.named_parameters() if p.requires_grad and p.grad is not None}
    return {k: np.float32(v.detach().cpu().numpy()) for k, v in losses.items()}, heads._last_state["aux"], grads


def _mean2(l0, l1):
    return np.float32((np.float64(l0) + np.float64(l1)) / np.float64(2.0))


@pytest.mark.parametrize("case", ["past_max_iter", "no_class_reaches_tau"])
def test_without_maps_losses_are_the_mean_and_gradients_the_average(case):
    """No image-gradient pass: past WSL.CSC_MAX_ITER (W = ones), and tau = 2.0 (no class active: W comes from zero maps through
    the weights op).  Both losses of the 2-image batch = fp32(((double)l_0 + (double)l_1) / 2) of two single-image forwards of
    the same weights, exactly; the head weight gradients = the average of the singles within 2e-3 relative (GEMM accumulation
    order: the batch's dW GEMMs sum over 37 more rows), with the 2e-6 floor tests/test_csc_gpu.py puts on this fixture for the
    det bias, whose gradient is identically zero."""
    _, model, a, b = _setup()
    it, tau, mx = (10, 0.7, 2) if case == "past_max_iter" else (1, 2.0, 100)
    singles = [_step(model, x, it, tau, mx) for x in (a, b)]
    model.roi_heads.enable_image_batches(True)
    losses, aux, grads = _step(model, a + b, it, tau, mx)
    assert sorted(losses) == ["loss_cls_neg", "loss_cls_pos"]
    if case == "past_max_iter":
        assert aux["W"] is None and aux["cpgs"] is None and singles[0][1]["W"] is None
    else:
        R0 = singles[0][1]["W"].shape[0]
        assert isinstance(aux["cpgs"], list) and len(aux["cpgs"]) == 2 and not any(bool(m.any()) for m in aux["cpgs"])
        assert torch.equal(aux["W"][:R0], singles[0][1]["W"]) and torch.equal(aux["W"][R0:], singles[1][1]["W"])
        assert aux["W"].shape[0] == R0 + 37
    for k in losses:
        want = _mean2(singles[0][0][k], singles[1][0][k])
        print(case, k, "batch %.9g  singles %.9g %.9g  defined mean %.9g" % (losses[k], singles[0][0][k], singles[1][0][k], want))
        assert losses[k] == want, (k, losses[k], want)
    assert grads and set(grads) == set(singles[0][2])
    for n_, g in grads.items():
        want = ((singles[0][2][n_].double() + singles[1][2][n_].double()) / 2.0).cpu().numpy()
        err = np.abs(g.double().cpu().numpy() - want).max()
        print(case, n_, "max |g - avg| %.3e of %.3e" % (err, np.abs(want).max()))
        assert err <= 2e-3 * np.abs(want).max() + 2e-6, (n_, err)


def _compare_image(tag, cpg, W, losses, ref_aux, ref_losses=None):
    """one image of the batch against its single-image step -> prints the differences and returns whether all were zero"""
    got, want = cpg.cpu().numpy(), ref_aux["cpgs"].cpu().numpy()
    assert got.shape == want.shape
    dm = np.abs(got - want)
    dW = np.abs(W.cpu().numpy() - ref_aux["W"].cpu().numpy())
    print("%s: maps max diff %.3e median %.3e frac > 5e-3 %.4f; W max diff %.3e median %.3e" % (
        tag, dm.max(), np.median(dm), (dm > 5e-3).mean(), dW.max(), np.median(dW)))
    return dm, dW


def test_with_maps_each_image_equals_its_single_image_step():
    """tau = 0, set_deterministic(True): every labelled class of both images gets its map from the batch's two slot passes.
    Per image, maps and W rows against that image's single-image step of the same weights: BIT EQUALITY.
    Measured on an MI355X (fp32, this fixture): maps max |diff| 0.0 and W max |diff| 0.0 for both images, both batch losses
    equal to the defined mean of the singles - the trunk's data-gradient kernels, the fc GEMMs and the deterministic RoIPool
    backward are batch-invariant here, so the bounds of tests/test_csc_gpu.py::test_csc_image_gradient_other_trunks are not needed."""
    _, model, a, b = _setup()
    singles = [_step(model, x, 1, 0.0, 100) for x in (a, b)]
    model.roi_heads.enable_image_batches(True)
    losses, aux, _ = _step(model, a + b, 1, 0.0, 100)
    R0 = singles[0][1]["W"].shape[0]
    rows = (slice(0, R0), slice(R0, R0 + 37))
    assert isinstance(aux["cpgs"], list) and len(aux["cpgs"]) == 2
    for i in range(2):
        ref = singles[i][1]
        active = [c for c in range(ref["cpgs"].shape[0]) if float(ref["cpgs"][c].max()) > 0]
        assert len(active) == 2 and [c for c in range(4) if float(aux["cpgs"][i][c].max()) > 0] == active
        dm, dW = _compare_image("image %d" % i, aux["cpgs"][i], aux["W"][rows[i]], losses, ref)
        assert dm.max() == 0.0 and dW.max() == 0.0, (i, dm.max(), dW.max())  # bit equality
    for k in losses:
        want = _mean2(singles[0][0][k], singles[1][0][k])
        print(k, "batch %.9g defined mean %.9g" % (losses[k], want))
        assert losses[k] == want, (k, losses[k], want)
    assert float(aux["W"].min()) < 0


def test_unequal_sizes_crop_per_image():
    """image 1 is a smaller crop: image 0 defines both padded dimensions, so its forward sees no padding and is held to the
    comparison above; image 1's maps have its own shape, are finite, and are normalised by the maximum of its own crop"""
    _, model, a, b = _setup(crop=(40, 48))
    H0, W0 = a[0]["image"].shape[1:]
    single, aux0, _ = _step(model, a, 1, 0.0, 100)
    model.roi_heads.enable_image_batches(True)
    losses, aux, _ = _step(model, a + b, 1, 0.0, 100)
    assert tuple(model.roi_heads.images.nhwc.shape[1:3]) == (H0, W0)
    K = aux0["cpgs"].shape[0]
    assert tuple(aux["cpgs"][0].shape) == (K, H0, W0) and tuple(aux["cpgs"][1].shape) == (K, 40, 48)
    R0 = aux0["W"].shape[0]
    dm, dW = _compare_image("image 0 beside a smaller image", aux["cpgs"][0], aux["W"][:R0], losses, aux0)
    assert dm.max() == 0.0 and dW.max() == 0.0, (dm.max(), dW.max())
    labelled = set(b[0]["instances"].gt_classes.tolist())
    m1 = aux["cpgs"][1]
    assert bool(torch.isfinite(m1).all()) and bool(torch.isfinite(aux["W"]).all())
    for c in range(K):
        assert float(m1[c].max()) == (1.0 if c in labelled else 0.0), c
        assert float(m1[c].min()) >= 0.0
    assert all(np.isfinite(v) for v in losses.values())


def test_trainer_window_of_two_image_batches():
    """one eager Trainer window with WSL.ITER_SIZE = 2 on 2-image batches (iterations 1, 2: the update closes the window) and
    the first step of the next one: the losses of all three steps equal the same steps run by hand, bit for bit"""
    out = []
    for mode in ("trainer", "hand"):
        cfg, model, a, b = _setup()
        batch = a + b
        heads = model.roi_heads
        heads.enable_image_batches(True)
        heads.tau, heads.csc_max_iter = 0.0, 100
        cfg.WSL.ITER_SIZE = 2
        opt = build_optimizer(cfg, model)
        got = []
        if mode == "trainer":
            tr = Trainer(cfg, model, iter([batch] * 5), optimizer=opt, start_iter=1)
            for _ in range(3):
                got.append({k: float(v.detach()) for k, v in tr.run_step().items()})
            assert opt._steps == 1
        else:
            opt.zero_grad()
            for it in (1, 2, 3):
                losses = model(batch)
                if not model.backward_losses(0.5):
                    (sum(losses.values()) / 2).backward()
                if it == 2:
                    opt.step()
                    opt.zero_grad()
                got.append({k: float(v.detach()) for k, v in losses.items()})
        torch.cuda.synchronize()
        assert len(heads._last_state["aux"]["cpgs"]) == 2
        out.append(got)
    for x, y in zip(*out):
        assert sorted(x) == ["loss_cls_neg", "loss_cls_pos"] and x == y, (x, y)
    assert out[0][2] != out[0][1]  # the window's update moved the weights


def test_refusals():
    """the default head still refuses a 2-image batch; a graphed step on the opted-in head is still refused"""
    cfg, model, a, b = _setup()
    heads = model.roi_heads
    assert heads.image_batches is False
    with pytest.raises(DrnError, match="ONE image per step"):
        model(a + b)
    heads.iter = 1
    heads.enable_image_batches(True)
    opt = build_optimizer(cfg, model)
    with pytest.raises(DrnError, match="eager steps only"):
        GraphedTrainStep(model, opt, a + b)
    with pytest.raises(DrnError, match="eager steps only"):
        GraphedTrainStep(model, opt, a)
