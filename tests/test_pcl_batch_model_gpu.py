"""PCLROIHeads on image batches (enable_image_batches): the head, the backward and the graphed step on a 2-image batch made
from the reference-generated fixture model_pcl_r50c4_tiny - its image, and the same image with its first 37 proposals and
another label vector."""
import numpy as np
import pytest
import torch

import golden_util as G
from __graft_entry__ import load_package

load_package()
from drn_wsod_pytorch_amd._cabi import DrnError  # noqa: E402
from drn_wsod_pytorch_amd.engine import GraphedTrainStep, build_optimizer  # noqa: E402

pytestmark = pytest.mark.gpu

NAME = "model_pcl_r50c4_tiny"


def _relerr(a, b, floor=1e-6):
    """tests/test_model_gpu.py::_relerr: max |a-b| relative to the scale of b"""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.abs(a - b).max() / (np.abs(b).max() + floor))


def _setup():
    """tests/test_model_gpu.py::_setup for the fp32 PCL fixture -> (model cfg, model, [image 0], [image 1])"""
    assert torch.cuda.is_available()
    load_package()
    ocfg = G.MODEL_CASES[NAME]
    d = G.load(NAME)
    cfg, model = G.drn_model(ocfg, int(d["seed"]), "cuda", 5, "fp32")
    masks = G.dropmasks_from(d)
    assert masks is None  # the fixture was generated with dropout patched to identity
    model.roi_heads.box_head.dropout_p = 0.0
    first = G.batch_from(d)[0]
    K = ocfg.num_classes
    other = [c for c in range(K) if c not in set(first["gt_classes"].tolist())]
    assert other, "the fixture labels every class: no other label vector"
    second = dict(first, proposal_boxes=first["proposal_boxes"][:37].clone(),
                  objectness_logits=first["objectness_logits"][:37].clone(),
                  gt_classes=torch.tensor(other[:2], dtype=first["gt_classes"].dtype),
                  gt_boxes=torch.zeros((len(other[:2]), 4)))
    assert len(first["proposal_boxes"]) > 37
    return cfg, model, G.drn_inputs([first]), G.drn_inputs([second])


def _refine_grads(model):
    return {n: p.grad.detach().clone() for n, p in model.named_parameters()
            if p.requires_grad and "box_refinery" in n and p.grad is not None}


def test_two_image_batch_refused_without_the_opt_in():
    _, model, a, b = _setup()
    model.train()
    assert model.roi_heads.image_batches is False
    with pytest.raises(DrnError, match="ONE image per step"):
        model(a + b)


def test_batch_losses_and_refinement_gradients_are_the_mean_over_images():
    """loss_cls_r{k} of the 2-image batch = fp32((double)l_0 + (double)l_1) / 2) of two single-image forward passes of the same
    weights; the refinement branches' weight gradients = the average of the two single-image gradients within 2e-3 relative -
    the fp32 bound tests/test_model_gpu.py::test_pcl_heads_two_steps_vs_oracle_fp32 puts on every gradient of this fixture
    (`_relerr(g, rg) < 2e-3`: GEMM accumulation order; the dW GEMM of the batch sums over 37 more rows than either single one)"""
    _, model, a, b = _setup()
    model.train()
    singles = []
    for x in (a, b):
        model.zero_grad()
        losses = model(x)
        sum(losses.values()).backward()
        torch.cuda.synchronize()
        singles.append(({k: v.detach().cpu().numpy().astype(np.float32) for k, v in losses.items()}, _refine_grads(model)))
    model.roi_heads.enable_image_batches(True)
    model.zero_grad()
    losses = model(a + b)
    sum(losses.values()).backward()
    torch.cuda.synchronize()
    assert set(losses) == set(singles[0][0])  # the loss names are unchanged
    targets = model.roi_heads._last_state["aux"]["targets"]
    refine = sorted(k for k in losses if k.startswith("loss_cls_r"))
    assert len(refine) == G.MODEL_CASES[NAME].refine_num and len(targets) == 2 and len(targets[0]) == len(refine)
    assert targets[0][0]["labels"].shape[0] == len(a[0]["proposals"]) and targets[1][0]["labels"].shape[0] == 37
    for k in refine:
        l0, l1 = singles[0][0][k], singles[1][0][k]
        want = np.float32((np.float64(l0) + np.float64(l1)) / np.float64(2.0))
        got = np.float32(losses[k].detach().cpu().numpy())
        print(k, "batch %.9g  singles %.9g %.9g  defined mean %.9g" % (got, l0, l1, want))
        assert got == want, (k, got, want)
    grads = _refine_grads(model)
    assert grads and set(grads) == set(singles[0][1])
    for n_, g in grads.items():
        want = (singles[0][1][n_].double() + singles[1][1][n_].double()) / 2.0
        err = _relerr(g.cpu().numpy(), want.cpu().numpy())
        print(n_, "relerr %.3e" % err)
        assert err < 2e-3, (n_, err)


def test_eager_and_graphed_steps_agree_on_a_two_image_batch():
    """three optimizer steps, eager against GraphedTrainStep captured on the opted-in head: the tolerance of the pinned
    single-image test (tests/test_model_gpu.py::test_pcl_heads_reject_batches_and_graph_capture_ok, 1e-6); opting in after
    the step was primed is refused"""
    res = []
    for mode in ("eager", "graph"):
        cfg, model, a, b = _setup()
        batch = a + b
        model.train()
        model.roi_heads.enable_image_batches(True)
        opt = build_optimizer(cfg, model)
        out = []
        if mode == "graph":
            stepper = GraphedTrainStep(model, opt, batch)
            for _ in range(3):
                out.append({k: float(v.detach()) for k, v in stepper.step(batch, batch).items()})
            with pytest.raises(DrnError, match="primed"):
                model.roi_heads.enable_image_batches(False)
            assert model.roi_heads.image_batches is True
        else:
            for _ in range(3):
                opt.zero_grad()
                losses = model(batch)
                sum(losses.values()).backward()
                opt.step()
                out.append({k: float(v.detach()) for k, v in losses.items()})
        torch.cuda.synchronize()
        res.append((out, {n: prm.detach().clone() for n, prm in model.named_parameters() if prm.requires_grad}))
    for x, y in zip(res[0][0], res[1][0]):
        assert set(x) == set(y)
        for k in x:
            assert abs(x[k] - y[k]) <= 1e-6 * max(1.0, abs(x[k])), (k, x[k], y[k])
    for n_ in res[0][1]:
        assert torch.allclose(res[0][1][n_], res[1][1][n_], rtol=0, atol=1e-6), n_


def test_opt_in_after_priming_is_refused():
    cfg, model, a, _ = _setup()
    model.train()
    opt = build_optimizer(cfg, model)
    stepper = GraphedTrainStep(model, opt, a)
    stepper.step(a, a)
    torch.cuda.synchronize()
    with pytest.raises(DrnError, match="primed"):
        model.roi_heads.enable_image_batches(True)
    assert model.roi_heads.image_batches is False
