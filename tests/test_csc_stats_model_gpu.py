"""CSCROIHeads.enable_csc_stats on the tiny WSR-18 CSC fixture of tests/test_csc_batch_model_gpu.py (model_csc_r18dc5_tiny: its
image, and the same image with its first 37 proposals and another label vector): the option changes nothing the step computes,
the collected table is the numpy restatement (tests/csc_stats_util.py) of the step's own scores, W, labels and active set, a
2-image batch counts what its two single-image steps count, and a step past CSC_MAX_ITER leaves the table alone.  fp32,
dropout off, deterministic RoIPool backward."""
import numpy as np
import pytest
import torch

import csc_stats_util as U
import golden_util as G
from __graft_entry__ import load_package

pkg = load_package()
from drn_wsod_pytorch_amd import metrics, ops  # noqa: E402

pytestmark = pytest.mark.gpu

NAME = "model_csc_r18dc5_tiny"
STEPS = ((1, 0.0), (2, 0.15), (3, 2.0))  # (head iteration, tau): every labelled class active / the fixture's own tau / none


@pytest.fixture(autouse=True)
def _deterministic():
    pkg.set_deterministic(True)
    yield
    pkg.set_deterministic(False)


def _setup():
    """-> (model, [image 0], [image 1]) as tests/test_csc_batch_model_gpu.py builds them"""
    ocfg = G.csc_case()
    d = G.load(NAME)
    _, model = G.drn_model(ocfg, int(d["seed"]), "cuda", 5, "fp32")
    heads = model.roi_heads
    heads.box_head.dropout_p = 0.0
    heads.csc_max_iter = 100
    model.train()
    first = G.batch_from(d)[0]
    other = [c for c in range(ocfg.num_classes) if c not in set(first["gt_classes"].tolist())]
    second = dict(first, proposal_boxes=first["proposal_boxes"][:37].clone(), objectness_logits=first["objectness_logits"][:37].clone(),
                  gt_classes=torch.tensor(other[:2], dtype=first["gt_classes"].dtype), gt_boxes=torch.zeros((len(other[:2]), 4)))
    return model, G.drn_inputs([first]), G.drn_inputs([second])


def _step(model, batch, it, tau):
    """one forward + backward at a fixed head iteration -> what the step computed, and what the restatement needs of it"""
    heads = model.roi_heads
    heads.iter, heads.tau = it, tau
    model.zero_grad()
    losses = model(batch)
    sum(losses.values()).backward()
    torch.cuda.synchronize()
    aux = heads._last_state["aux"]
    sched = heads._csc_sched
    if isinstance(sched, ops.CscBatchPlan):
        active = {(i, c) for row in sched.slots for i, c in enumerate(row) if c >= 0}
    else:
        active = {(0, c) for c in (sched or [])}
    cpgs = aux["cpgs"] if isinstance(aux["cpgs"], (list, type(None))) else [aux["cpgs"]]
    return dict(losses={k: v.detach().clone() for k, v in losses.items()},
                W=None if aux["W"] is None else aux["W"].clone(), scores=aux["scores"].clone(),
                cpgs=None if cpgs is None else [m.clone() for m in cpgs], active=active,
                grads={n: p.grad.detach().clone() for n, p in model.named_parameters() if p.requires_grad and p.grad is not None})


def _onehot(batch, K):
    oh = np.zeros((len(batch), K), np.float32)
    for i, x in enumerate(batch):
        oh[i, x["instances"].gt_classes.tolist()] = 1.0
    return oh


def _off(batch):
    return np.concatenate([[0], np.cumsum([len(x["proposals"]) for x in batch])]).astype(np.int32)


def _restate(t, out, batch, K):
    return U.add_step(t, out["scores"].cpu().numpy(), out["W"].cpu().numpy(), _off(batch), _onehot(batch, K), out["active"],
                      round32=False)


def test_three_steps_are_bit_equal_with_the_option_on_and_the_table_is_the_restatement():
    model, a, _ = _setup()
    heads = model.roi_heads
    K = heads.num_classes
    off = [_step(model, a, it, tau) for it, tau in STEPS]
    st = heads.enable_csc_stats(period=1000, start_iter=1)
    on = [_step(model, a, it, tau) for it, tau in STEPS]
    assert heads._engine.csc_stats is st and st.cur_iter == 4 and st.blocks == []
    for x, y in zip(off, on):
        assert sorted(x["losses"]) == ["loss_cls_neg", "loss_cls_pos"]
        for k in x["losses"]:
            assert torch.equal(x["losses"][k], y["losses"][k]), k
        assert torch.equal(x["W"], y["W"]) and torch.equal(x["scores"], y["scores"]) and x["active"] == y["active"]
        assert len(x["cpgs"]) == len(y["cpgs"]) and all(torch.equal(m, n) for m, n in zip(x["cpgs"], y["cpgs"]))
        assert x["grads"] and set(x["grads"]) == set(y["grads"])
        for n_, g in x["grads"].items():
            assert torch.equal(g, y["grads"][n_]), n_
    assert [len(x["active"]) for x in on] == [2, len(on[1]["active"]), 0] and float(on[0]["W"].min()) < 0
    ref = U.new_table(K)
    for out in on:
        _restate(ref, out, a, K)
    (it, got), = st.flush()
    assert it == 3 and got["steps"] == 3 and got["num_img"] == 3
    U.assert_close(got, ref, "three steps")
    assert got["csc_label"].sum() == sum(len(x["active"]) for x in on) and got["ori_label"].sum() == 3 * int(_onehot(a, K).sum())
    text = st.blocks[-1][1]
    assert text == metrics.CscStats.format(got, 3) and text.count("\n") == K + 2
    # a step past CSC_MAX_ITER: W is None, the forward is counted, the table stays as the drain left it
    before = st.table.clone()
    heads.csc_max_iter = 2
    out = _step(model, a, 10, 0.15)
    assert out["W"] is None and st.cur_iter == 5
    assert torch.equal(st.table, before) and not bool(before.any())
    heads.disable_csc_stats()
    assert heads._engine.csc_stats is None


def test_a_two_image_batch_counts_what_its_single_image_steps_count():
    model, a, b = _setup()
    heads = model.roi_heads
    K = heads.num_classes
    st = heads.enable_csc_stats(period=1000, start_iter=1)
    tables = []
    for batch in (a, b, a + b):
        heads.enable_image_batches(len(batch) > 1)
        out = _step(model, batch, 1, 0.0)
        (_, got), = st.flush()
        U.assert_close(got, _restate(U.new_table(K), out, batch, K), "%d image(s)" % len(batch))
        tables.append((got, out))
    (ta, _), (tb, _), (tab, out) = tables
    assert tab["num_img"] == 2 and tab["steps"] == 1 and ta["steps"] + tb["steps"] == 2
    assert len(out["active"]) == 4 and tab["csc_label"].sum() == 4
    for f in U.INT_FIELDS:
        assert np.array_equal(tab[f], ta[f] + tb[f]), (f, tab[f], ta[f], tb[f])
    bound = _restate(U.new_table(K), out, a + b, K)
    for f in U.FP_FIELDS:
        err = np.abs(tab[f] - (ta[f] + tb[f]))
        print(f, "max |batch - (single + single)| %.3g" % err.max())
        assert np.all(err <= bound["bound_" + f]), (f, tab[f], ta[f] + tb[f])
