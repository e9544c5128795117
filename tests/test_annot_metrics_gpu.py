"""The annotated-box block of the per-step metrics on the device (include/drn_wsod.h "per-step metrics"):
  1. drn_label_proposals against the restatement of tests/annot_metrics_util.py - labels, matched and counts equal exactly - over
     M x images x annotated boxes per image x K x Matcher settings, on an integer grid with IoU exactly at a threshold, identical
     annotated boxes, zero-area boxes and proposals equal to an annotated box;
  2. drn_mil_metrics against the restatement, exact, K = 1 and equal top scores included; the three launches captured and replayed;
  3. through the model: the reference fixture's two steps (eager Trainer and GraphedTrainStep, fp32), one step of the tiny WSDDN,
     PCL and CSC models against the restatement on the model's own MIL scores, and the option off = today's records and launches."""
import numpy as np
import pytest
import torch

import annot_metrics_util as AU
import golden_util as G
import metrics_util as MU
from __graft_entry__ import load_package

pytestmark = pytest.mark.gpu
DEV = "cuda"
W = 72
MAX_GT = 24
MS = (1, 63, 64, 65, 129, 200, 700)  # 700: more than one workgroup (256 rows) per image
GS = (0, 1, 2, 17, MAX_GT)
KS = (1, 2, 20, 80)
MATCHERS = (((0.5,), (0, 1)), ((0.1, 0.5), (-1, 0, 1)))


@pytest.fixture(scope="module")
def drn():
    assert torch.cuda.is_available(), "GPU tests need a GPU (run with -m gpu on the MI355X box)"
    pkg = load_package()
    pkg._cabi.lib()
    import importlib

    return importlib.import_module("drn_wsod_pytorch_amd.ops")


@pytest.fixture(autouse=True)
def _fp32_after():
    yield
    load_package().set_precision("fp32")


# ------------------------------------------------------------------------------------------------------ 1. drn_label_proposals
def _split(M, n_img):
    """unequal rows per image (an image may get none)"""
    w = np.arange(1, n_img + 1, dtype=np.float64) ** 2
    cuts = np.floor(np.cumsum(w) / w.sum() * M).astype(np.int64)
    cuts[-1] = M
    return [0] + cuts.tolist()


def _boxes(rs, n):
    """integer-grid boxes, a few of them with zero area"""
    x0, y0 = rs.randint(0, 9, size=n), rs.randint(0, 9, size=n)
    w, h = rs.randint(0, 6, size=n), rs.randint(0, 6, size=n)
    w[rs.rand(n) < 0.8] += 1  # ~20 % keep a chance of zero width / height
    return np.stack([x0, y0, x0 + w, y0 + h], 1).astype(np.float32)


def _label_case(rs, M, n_img, g0, K):
    off = _split(M, n_img)
    props = _boxes(rs, M)
    per_b, per_c = [], []
    for i in range(n_img):
        Gn = GS[(GS.index(g0) + i) % len(GS)]
        b = _boxes(rs, Gn)
        r0, r1 = off[i], off[i + 1]
        if Gn >= 1:
            b[0] = [0, 0, 2, 1]
        if Gn >= 2:
            b[1] = b[0]  # two identical annotated boxes: the lower index must win
        if Gn >= 3:
            b[2] = [0, 0, 1, 1]
        if Gn >= 5:
            b[Gn - 1] = b[3]  # and a later identical pair
        per_b.append(b)
        per_c.append(rs.randint(0, K, size=Gn))
        rows = list(range(r0, r1))
        plant = [[0, 0, 2, 2], [0, 0, 10, 1], [0, 0, 2, 1], [4, 4, 4, 7]]  # IoU 0.5 and 0.1 exactly, equal to a box, zero area
        for r, p in zip(rows, plant):
            props[r] = p
        if Gn and len(rows) > 4:
            props[rows[4]] = b[Gn - 1]  # a proposal equal to the LAST annotated box
    gb, gc, cnt = AU.pack(per_b, per_c, MAX_GT)
    return props, off, gb, gc, cnt


def _dev(*arrs):
    return [torch.from_numpy(np.ascontiguousarray(a)).to(DEV) for a in arrs]


@pytest.mark.parametrize("n_img", [1, 2, 4])
@pytest.mark.parametrize("thr,lab", MATCHERS)
def test_label_proposals_exact_over_the_grid(drn, thr, lab, n_img):
    rs = np.random.RandomState(100 * n_img + len(thr))
    seen = set()
    for M in MS:
        for g0 in GS:
            for K in KS:
                props, off, gb, gc, cnt = _label_case(rs, M, n_img, g0, K)
                want_l, want_m, want_c = AU.label_proposals(props, off, gb, gc, cnt, K, thr, lab)
                dp, do, dgb, dgc, dcnt = _dev(props, np.array(off, dtype=np.int32), gb, gc, cnt)
                counts = torch.zeros((8,), dtype=torch.int32, device=DEV)
                out = drn.label_proposals(dp, do, n_img, dgb, dgc, dcnt, K, thr, lab, counts=counts,
                                          max_rows=max(b - a for a, b in zip(off, off[1:])))
                tag = (M, n_img, g0, K, thr)
                assert np.array_equal(out["labels"].cpu().numpy().astype(np.int64), want_l), tag
                assert np.array_equal(out["matched"].cpu().numpy().astype(np.int64), want_m), tag
                c = counts.cpu().numpy().astype(np.int64)
                assert np.array_equal(c[:3], want_c) and not c[3:].any() and c[:3].sum() == M, (tag, c, want_c)
                seen.update(np.unique(want_l).tolist())
    assert K in seen and 0 in seen and ((-1 in seen) == (-1 in lab))


def test_label_proposals_planted_edges(drn):
    """the hand-made case of the CPU test on the device, with the labels written out: IoU exactly 0.5 and 0.1 sit on the closed
    side of their interval, identical boxes match the lower index, a zero-area proposal overlaps nothing"""
    props = np.array([[0, 0, 2, 2], [0, 0, 2, 1], [5, 5, 5, 9], [0, 0, 10, 1], [20, 20, 30, 30]], dtype=np.float32)
    gb, gc, cnt = AU.pack([[[0, 0, 2, 1], [0, 0, 2, 1], [0, 0, 1, 1]]], [[3, 1, 2]], 64)
    dp, do, dgb, dgc, dcnt = _dev(props, np.array([0, 5], dtype=np.int32), gb, gc, cnt)
    out = drn.label_proposals(dp, do, 1, dgb, dgc, dcnt, 7, (0.5,), (0, 1))
    assert out["labels"].tolist() == [3, 3, 7, 7, 7] and out["matched"].tolist() == [0] * 5 and out["counts"].tolist()[:3] == [0, 3, 2]
    out = drn.label_proposals(dp, do, 1, dgb, dgc, dcnt, 7, (0.1, 0.5), (-1, 0, 1), counts=out["counts"])  # counts are ADDED to
    assert out["labels"].tolist() == [3, 3, -1, 7, -1] and out["counts"].tolist()[:3] == [2, 4, 4]
    # only [0, 0, 1, 1]: the long proposal has IoU exactly 0.1 - background, not ignored
    gb, gc, cnt = AU.pack([[[0, 0, 1, 1]]], [[2]], 64)
    dgb, dgc, dcnt = _dev(gb, gc, cnt)
    out = drn.label_proposals(dp, do, 1, dgb, dgc, dcnt, 7, (0.1, 0.5), (-1, 0, 1))
    assert out["labels"].tolist() == [7, 2, -1, 7, -1]  # IoU 0.25, 0.5, 0, 0.1, 0
    want = AU.label_proposals(props, [0, 5], gb, gc, cnt, 7, (0.1, 0.5), (-1, 0, 1))
    assert out["labels"].tolist() == want[0].tolist()


def test_label_proposals_refuses(drn):
    from drn_wsod_pytorch_amd._cabi import DrnError

    props = np.zeros((3, 4), dtype=np.float32)
    gb, gc, cnt = AU.pack([[]], [[]], drn.LABEL_MAX_GT + 1)
    dp, do, dgb, dgc, dcnt = _dev(props, np.array([0, 3], dtype=np.int32), gb, gc, cnt)
    with pytest.raises(DrnError):
        drn.label_proposals(dp, do, 1, dgb, dgc, dcnt, 5)
    gb, gc, cnt = AU.pack([[]], [[]], drn.LABEL_MAX_GT)  # the largest block that is built; no annotated box: all background
    dgb, dgc, dcnt = _dev(gb, gc, cnt)
    out = drn.label_proposals(dp, do, 1, dgb, dgc, dcnt, 5)
    assert out["labels"].tolist() == [5, 5, 5] and out["matched"].tolist() == [0, 0, 0] and out["counts"].tolist()[:3] == [0, 3, 0]
    with pytest.raises(DrnError):
        drn.label_proposals(dp, do, 1, dgb, dgc, dcnt, 5, (0.1, 0.2, 0.3, 0.4), (0, 0, 0, 0, 1))


# ----------------------------------------------------------------------------------------------------------- 2. drn_mil_metrics
def _mil_case(rs, M, K):
    x = rs.rand(M, K).astype(np.float32) * np.float32(1e-2)
    g = rs.randint(-1, K + 1, size=M).astype(np.int32)
    for r in range(0, M, 2):  # about half the rows predict their label
        if 0 <= g[r] < K:
            x[r, g[r]] = 0.5 + rs.rand()
    for i, r in enumerate(range(1, M, 7)):  # equal top scores: the first index wins
        if K >= 2:
            a, b = sorted(rs.choice(K, 2, replace=False))
            x[r] = 0.0
            x[r, a] = x[r, b] = 0.75
            g[r] = (a, b, K - 1, K)[i % 4]
    return x, g


@pytest.mark.parametrize("K", KS)
def test_mil_metrics_exact(drn, K):
    rs = np.random.RandomState(7 + K)
    for M in MS:
        x, g = _mil_case(rs, M, K)
        want = AU.mil_counts(x, g, M)
        dg = torch.from_numpy(g).to(DEV)
        wide = np.full((M + 2, K + 5), np.nan, dtype=np.float32)  # every cell the kernel must not read is NaN
        wide[:M, :K] = x
        for xd in (torch.from_numpy(x).to(DEV), torch.from_numpy(wide).to(DEV)[:, :K]):
            counts = torch.zeros((8,), dtype=torch.int32, device=DEV)
            drn.mil_metrics(xd, dg, M, counts)
            c = counts.cpu().numpy().astype(np.int64)
            assert np.array_equal(c[3:7], want) and not c[:3].any() and c[7] == 0, (M, K, c, want)
        if K == 1:
            assert want[1:].tolist() == [0, 0, 0]
        elif M >= 63:
            assert want[3] > 0 and want[1] > 0


def test_block_launches_captured_and_replayed(drn):
    """label_proposals + mil_metrics + metrics_record(annot) as a captured graph: two replays with changed boxes and scores give two
    records with the changed block; a record written by the plain entry point has zeros where the block would be"""
    from drn_wsod_pytorch_amd.metrics import decode_record

    K, n_img, M = 5, 2, 300
    rs = np.random.RandomState(3)
    props, off, gb, gc, cnt = _label_case(rs, M, n_img, 17, K)
    x, _ = _mil_case(rs, M, K)
    dp, do, dgb, dgc, dcnt, dx = _dev(props, np.array(off, dtype=np.int32), gb, gc, cnt, x)
    lab, mat = torch.zeros(M, dtype=torch.int32, device=DEV), torch.zeros(M, dtype=torch.int32, device=DEV)
    loss = [torch.full((1,), 0.5, device=DEV)]
    r = drn.metrics_ring(4, DEV)
    block = r["counts"][drn.METRICS_ANNOT_ROW]

    def trio():
        drn.label_proposals(dp, do, n_img, dgb, dgc, dcnt, K, counts=block, out=(lab, mat))
        drn.mil_metrics(dx, lab, M, block)
        drn.metrics_record(loss, r["counts"], 0, M, r["ring"], r["state"], annot=True)

    drn.metrics_record(loss, r["counts"], 0, M, r["ring"], r["state"])  # record 0: no block
    trio()                                                                # record 1, eagerly
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        trio()
    want = [(props, gb, gc, cnt, x)]
    for _ in range(2):
        p2, _, gb2, gc2, cnt2 = _label_case(rs, M, n_img, 2, K)
        x2, _ = _mil_case(rs, M, K)
        for dst, src in ((dp, p2), (dgb, gb2), (dgc, gc2), (dcnt, cnt2), (dx, x2)):
            dst.copy_(torch.from_numpy(src))
        g.replay()
        want.append((p2, gb2, gc2, cnt2, x2))
    host = r["buf"].cpu().numpy()
    assert host[0] == 4 and not r["counts"].cpu().numpy().any()
    rec0 = host[4: 4 + W].astype(np.int64) & 0xFFFFFFFF
    assert not rec0[20:71].any() and set(decode_record(rec0.tolist(), ["l"], n_img)) == {"l", "total_loss"}
    for i, (p, b, c, n, xs) in enumerate(want, start=1):
        rec = host[4 + (i % 4) * W: 4 + (i % 4 + 1) * W].astype(np.int64) & 0xFFFFFFFF
        wl, _, wc = AU.label_proposals(p, off, b, c, n, K)
        wm = AU.mil_counts(xs, wl, M)
        assert rec[0] == i and rec[W - 1] == i and rec[2] == 0 and rec[70] == 1 and rec[69] == 0
        assert rec[62:65].tolist() == wc.tolist() and rec[65:68].tolist() == wm[:3].tolist() and rec[68] == wm[3], i
        assert not rec[20:62].any()
        got = decode_record(rec.tolist(), ["l"], n_img)
        assert {k: got[k] for k in AU.NAMES if k in got} == AU.scalars(wc, wm, M, n_img)
    assert len({tuple(host[4 + s * W + 62: 4 + s * W + 69]) for s in (1, 2, 3)}) == 3  # the three blocks differ


# ------------------------------------------------------------------------------------------------------- 3. through the model
def _restate(model, batch, ring, M, n_img):
    """the six scalars from the restatement, fed with the step's own MIL scores and the batch's annotated boxes"""
    heads = model.roi_heads
    K = heads.num_classes
    props = np.concatenate([b["proposals"].proposal_boxes.tensor.cpu().numpy() for b in batch])
    off = np.cumsum([0] + [len(b["proposals"]) for b in batch])
    gb, gc, cnt = AU.pack([b["instances"].gt_boxes.tensor.cpu().numpy() for b in batch],
                          [b["instances"].gt_classes.cpu().numpy() for b in batch], ring.max_gt)
    pm = heads.proposal_matcher
    labels, matched, counts = AU.label_proposals(props, off, gb, gc, cnt, K, pm.thresholds[1:-1], pm.labels)
    assert np.array_equal(ring.annot_labels.cpu().numpy(), labels) and np.array_equal(ring.annot_matched.cpu().numpy(), matched)
    scores = heads._last_state["aux"]["scores"].cpu().numpy()
    assert scores.shape == (M, K)
    return AU.scalars(counts, AU.mil_counts(scores, labels, M), M, n_img)


def _gold_model():
    gold = G.load("metrics_annot_r50c4_tiny")
    assert float(gold["min_margin"]) >= 1e-3
    ocfg = G.MODEL_CASES["model_r50c4_tiny"]
    cfg, model = G.drn_model(ocfg, int(gold["seed"]), DEV, 5, "fp32")
    model.roi_heads.box_head.dropout_p = 0.0  # the fixture was generated with dropout patched to identity
    model.train()
    return gold, cfg, model, G.drn_inputs(G.batch_from(gold))


def _check_gold(gold, recs):
    """every stored scalar of every step equal (integers over integers: the same division), present where the reference logged it"""
    steps = int(gold["steps"])
    assert [it for it, _ in recs] == list(range(steps))
    for s in range(steps):
        rec = recs[s][1]
        for k, v, p in zip([str(n) for n in gold["names"]], gold["step%d" % s], gold["present%d" % s]):
            assert (k in rec) == bool(p), (k, s)
            if p:
                assert rec[k] == float(v), (k, s, rec[k], float(v))
        assert "fast_rcnn/cls_accuracy_r0" in rec  # the branches' scalars stay beside the block


def test_reference_fixture_eager():
    from drn_wsod_pytorch_amd.engine import Trainer

    gold, cfg, model, batch = _gold_model()
    steps = int(gold["steps"])
    tr = Trainer(cfg, model, iter([batch] * (steps + 2)), metrics_period=steps, metrics_slots=4, metrics_annotated=True,
                 metrics_max_gt=8)
    for _ in range(steps):
        tr.run_step()
    ring = tr.metrics
    ring.drain()
    recs, lost = ring.collect(wait=True)
    assert lost == 0
    _check_gold(gold, recs)
    M = sum(len(b["proposals"]) for b in batch)
    want = _restate(model, batch, ring, M, len(batch))
    assert {k: recs[-1][1][k] for k in want} == want


def test_reference_fixture_graphed_step():
    from drn_wsod_pytorch_amd.engine import GraphedTrainStep, build_optimizer

    gold, cfg, model, batch = _gold_model()
    opt = build_optimizer(cfg, model)
    ring = model.roi_heads.enable_metrics(slots=4, annotated=True, max_gt=8)
    stepper = GraphedTrainStep(model, opt, batch)
    n_img, K = len(batch), model.roi_heads.num_classes
    assert stepper._gt_block.numel() == 2 * n_img * K + n_img + n_img * 8 * 5 + n_img  # the boxes ride in the label block
    for _ in range(int(gold["steps"])):
        stepper.step(batch, batch)
    ring.drain()
    recs, lost = ring.collect(wait=True)
    torch.cuda.synchronize()
    stepper.release()
    assert lost == 0
    _check_gold(gold, recs)


def _head_case(kind):
    from drn_wsod_pytorch_amd.engine import build_optimizer

    if kind == "csc":
        ocfg, d = G.csc_case(), G.load("model_csc_r18dc5_tiny")
    else:
        name = "model_%s_r50c4_tiny" % kind
        ocfg, d = G.MODEL_CASES[name], G.load(name)
    cfg, model = G.drn_model(ocfg, int(d["seed"]), DEV, 5, "fp32")
    model.roi_heads.box_head.dropout_p = 0.0
    if kind == "csc":
        model.roi_heads.tau, model.roi_heads.iter = float(d["tau"]), int(d["iter0"])
    model.train()
    return cfg, model, build_optimizer(cfg, model), G.drn_inputs(G.batch_from(d))


@pytest.mark.parametrize("kind,mode", [("wsddn", "eager"), ("wsddn", "graph"), ("pcl", "eager"), ("pcl", "graph"), ("csc", "eager")])
def test_other_heads_one_step_against_the_restatement(kind, mode):
    from drn_wsod_pytorch_amd.engine import GraphedTrainStep

    cfg, model, opt, batch = _head_case(kind)
    assert type(model.roi_heads).__name__ == {"wsddn": "WSDDNROIHeads", "pcl": "PCLROIHeads", "csc": "CSCROIHeads"}[kind]
    ring = model.roi_heads.enable_metrics(slots=4, annotated=True, max_gt=8)
    M, n_img = sum(len(b["proposals"]) for b in batch), len(batch)
    if mode == "graph":
        stepper = GraphedTrainStep(model, opt, batch)
        stepper.step(batch, batch)  # the priming step: eager
        stepper.step(batch, batch)  # a replay
    else:
        opt.zero_grad()
        sum(model(batch).values()).backward()
        opt.step()
    torch.cuda.synchronize()
    if mode == "graph":
        model.roi_heads._last_state = stepper.last_state
    want = _restate(model, batch, ring, M, n_img)
    ring.drain()
    recs, lost = ring.collect(wait=True)
    if mode == "graph":
        stepper.release()
    assert lost == 0 and len(recs) == (2 if mode == "graph" else 1)
    rec = recs[-1][1]
    assert {k: rec[k] for k in AU.NAMES if k in rec} == want and len(want) >= 4
    assert not any(k.endswith("_r0") for k in rec if k.startswith("fast_rcnn/"))  # these heads log no branch accuracy


def _spy_run(enable, steps=2):
    """the fixture's steps on the eager Trainer -> (loss bits per step, ring words, names of the C calls of the last step, decoded)"""
    from drn_wsod_pytorch_amd import _cabi
    from drn_wsod_pytorch_amd.engine import Trainer

    gold, cfg, model, batch = _gold_model()
    tr = Trainer(cfg, model, iter([batch] * (steps + 2)))
    ring = enable(model.roi_heads)
    calls, real = [], _cabi.call

    def spy(fn, *a):
        calls.append(fn)
        return real(fn, *a)

    _cabi.call = spy
    try:
        bits = []
        for _ in range(steps):
            mark = len(calls)
            ld = tr.run_step()
            torch.cuda.synchronize()
            bits.append({k: MU.f32_bits(v.detach().cpu().numpy()) for k, v in ld.items()})
    finally:
        _cabi.call = real
    ring.drain()
    recs, lost = ring.collect(wait=True)
    assert lost == 0
    return bits, ring.host.clone().numpy(), calls[mark:], recs


def test_option_off_is_todays_step():
    """enable_metrics(annotated=False) = enable_metrics(): the same launches, the same ring words, records that decode to today's
    names; annotated=True adds its three entry points and the block's words and changes no loss bit and no other record word"""
    new = ("drn_label_proposals", "drn_mil_metrics", "drn_metrics_record_annot")
    base = _spy_run(lambda h: h.enable_metrics(slots=4))
    off = _spy_run(lambda h: h.enable_metrics(slots=4, annotated=False, max_gt=8))
    on = _spy_run(lambda h: h.enable_metrics(slots=4, annotated=True, max_gt=8))
    assert off[0] == base[0] and on[0] == base[0]
    assert np.array_equal(off[1], base[1]) and off[2] == base[2] and not any(c in base[2] for c in new)
    assert [r for _, r in off[3]] == [r for _, r in base[3]] and not any(k in off[3][0][1] for k in AU.NAMES)
    assert [c for c in on[2] if c not in new[:2]] == [c if c != "drn_metrics_record" else new[2] for c in base[2]]
    assert [on[2].count(c) for c in new] == [1, 1, 1] and "drn_metrics_record" not in on[2]
    a, b = on[1].copy(), base[1].copy()
    for s in range(4):
        a[4 + s * W + 62: 4 + s * W + 71] = 0
        assert not b[4 + s * W + 62: 4 + s * W + 71].any()
    assert np.array_equal(a, b)
    for (_, ra), (_, rb) in zip(on[3], base[3]):
        assert {k: v for k, v in ra.items() if k not in AU.NAMES} == rb and all(k in ra for k in AU.NAMES[:4])


def test_graphed_step_without_the_option_keeps_its_label_block():
    from drn_wsod_pytorch_amd._cabi import DrnError
    from drn_wsod_pytorch_amd.engine import GraphedTrainStep, build_optimizer

    gold, cfg, model, batch = _gold_model()
    opt = build_optimizer(cfg, model)
    model.roi_heads.enable_metrics(slots=4, annotated=False)
    stepper = GraphedTrainStep(model, opt, batch)
    n_img, K = len(batch), model.roi_heads.num_classes
    stepper.step(batch, batch)
    assert stepper._gt_block.numel() == 2 * n_img * K + n_img and "ann_boxes" not in stepper.gt
    with pytest.raises(DrnError, match="after a graphed step was primed"):
        model.roi_heads.enable_metrics(annotated=True)
    torch.cuda.synchronize()
    stepper.release()
    # more annotated boxes than max_gt: refused on the host, before anything is launched
    ring = model.roi_heads.enable_metrics(slots=4, annotated=True, max_gt=1)
    many = [b for b in batch if len(b["instances"]) > 1]
    if many:
        with pytest.raises(DrnError, match="annotated boxes"):
            model(batch)
    torch.cuda.synchronize()
