"""The per-step metrics ring on the device (include/drn_wsod.h "per-step metrics"):
  1. drn_head_metrics against the int64 restatement of tests/metrics_util.py over a grid of M x (K + 1) x nh, with NaN / inf in every
     column and row the kernel must not read, degenerate label sets and planted arg-max ties - every integer equal;
  2. drn_metrics_record: six calls on a four-slot ring, and the pair of launches captured in a hipGraph and replayed with changed
     input contents;
  3. through the model on the eager Trainer (OICR chained path, the reg/ per-head path, WSDDN with no branch; fp32, bf16): metrics
     on and off give the same loss and parameter bits, off issues neither launch, and the drained records equal the step's own
     loss tensors and the restatement on the step's own logits and labels;
  4. GraphedTrainStep, 12 steps on an 8-slot ring drained twice without any synchronisation: the records equal a run that
     synchronises and reads `losses` after every step; GraphedFullStep (trainable trunk, deterministic mode) likewise;
  5. against the unmodified reference: tests/golden/metrics_r50c4_tiny.npz (gen_golden_metrics.py), every *_r{k} scalar equal;
  6. with the anomaly guard skipping a NaN step: the record carries the NaN, the parameters equal the guard-only run."""
import os

import numpy as np
import pytest
import torch

import golden_util as G
import metrics_util as MU
from __graft_entry__ import load_package

pytestmark = pytest.mark.gpu
DEV = "cuda"
NAN, INF = float("nan"), float("inf")
W = 72


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


def _i32(t):
    return t.view(torch.int32) if t.element_size() == 4 else t.view(torch.int16)


# ------------------------------------------------------------------------------------------------------ 1. drn_head_metrics
def _case(rs, M, K, nh, labels_kind):
    """logits [M + 3, ldl] with the branches at staggered columns (every 16-byte misalignment occurs), labels per branch, and the
    mask of the cells the kernel may read"""
    ncol = K + 1
    col0s = [3 + k * (ncol + 2 + (k % 3)) for k in range(nh)]
    ldl = col0s[-1] + ncol + 5
    rows = M + 3
    x = rs.standard_normal((rows, ldl)).astype(np.float32)
    used = np.zeros((rows, ldl), dtype=bool)
    for c0 in col0s:
        used[:M, c0: c0 + ncol] = True
    labels = []
    for k in range(nh):
        if labels_kind == "mixed":
            g = rs.randint(-1, K + 1, size=M)
        elif labels_kind == "ignore":
            g = np.full(M, -1)
        elif labels_kind == "bg":
            g = np.full(M, K)
        else:
            g = rs.randint(0, K, size=M)
        labels.append(g.astype(np.int32))
    # about half the rows predict their label (so the accuracy counters are not all near zero)
    for k, c0 in enumerate(col0s):
        for r in range(0, M, 2):
            if labels[k][r] >= 0:
                x[r, c0 + labels[k][r]] = 9.0 + rs.rand()
    # planted ties and extreme values, in branch (r % nh) of a few rows
    plant = list(range(M))[:12]
    setg = labels_kind == "mixed"  # (the degenerate label sets stay as they are: only the logits are planted)
    for i, r in enumerate(plant):
        k = r % nh
        c0, g = col0s[k], labels[k]
        row = x[r, c0: c0 + ncol]
        kind = i % 6
        if kind == 0:  # the maximum twice, at (c, K), label c: accurate, not a false negative
            c = int(rs.randint(0, K))
            row[:] = -1.0
            row[c] = row[K] = 7.5
            g[r] = c if setg else g[r]
        elif kind == 1 and K >= 2:  # the maximum twice, at (c', c), c' < c = label: not accurate
            c = int(rs.randint(1, K))
            cp = int(rs.randint(0, c))
            row[:] = -1.0
            row[cp] = row[c] = 7.5
            g[r] = c if setg else g[r]
        elif kind == 2:  # +0 / -0: a tie, the first index wins
            row[:] = -2.0
            a, b = sorted(rs.choice(ncol, 2, replace=False))
            row[a], row[b] = -0.0, 0.0
            g[r] = (a if a < K else K) if setg else g[r]
        elif kind == 3:
            row[:] = -2.0
            a, b = sorted(rs.choice(ncol, 2, replace=False))
            row[a], row[b] = 0.0, -0.0
            g[r] = (b if b < K else K) if setg else g[r]
        elif kind == 4:  # near the ends of the fp32 range
            row[:] = -3.0e38
            row[int(rs.randint(0, ncol))] = 3.0e38
            row[int(rs.randint(0, ncol))] = 3.2e38
        else:
            row[:] = -3.2e38
            a = int(rs.randint(0, ncol))
            row[a] = -3.0e38
            g[r] = min(a, K) if setg else g[r]
    return x, used, col0s, ldl, labels


def _hm_run(drn, x, col0s, K, labels, M):
    counts = torch.zeros((8, 8), dtype=torch.int32, device=DEV)
    drn.head_metrics(torch.from_numpy(x).to(DEV), col0s, K, labels, M, counts)
    return counts.cpu().numpy()


@pytest.mark.parametrize("nh", [1, 3, 8])
@pytest.mark.parametrize("ncol", [2, 6, 21, 81])
def test_head_metrics_exact_over_the_grid(drn, ncol, nh):
    K = ncol - 1
    rpw, rpb = drn.head_metrics_rows(K)
    Ms = sorted({1, 2, 2003, rpw - 1, rpw, rpw + 1, rpb - 1, rpb, rpb + 1} - {0})
    rs = np.random.RandomState(1000 * ncol + nh)
    for M in Ms:
        kinds = ("mixed", "ignore", "bg", "fg") if M in (2, rpb + 1, 2003) else ("mixed",)
        for kind in kinds:
            x, used, col0s, ldl, labels = _case(rs, M, K, nh, kind)
            want = MU.head_counts(x, col0s, K, labels, M)
            dev_labels = [torch.from_numpy(g).to(DEV) for g in labels]
            got = {}
            for fill in (NAN, INF, -INF):  # every cell the kernel must not read: unused columns, rows >= M
                xf = np.where(used, x, np.float32(fill)).astype(np.float32)
                got[fill] = _hm_run(drn, xf, col0s, K, dev_labels, M)
            tag = (M, ncol, nh, kind)
            assert np.array_equal(got[NAN][:nh, :6].astype(np.int64), want), (tag, got[NAN][:nh, :6], want)
            assert not got[NAN][nh:].any() and not got[NAN][:, 6:].any(), tag
            assert np.array_equal(got[NAN], got[INF]) and np.array_equal(got[NAN], got[-INF]), tag
            # the contiguous [nh, M] label form = the separate-pointer form
            both = torch.from_numpy(np.stack(labels)).to(DEV)
            xf = np.where(used, x, np.float32(NAN)).astype(np.float32)
            assert np.array_equal(_hm_run(drn, xf, col0s, K, both, M), got[NAN]), tag
            if kind == "mixed" and M == 2003:
                assert want[:, 2].sum() > 0 and want[:, 0].sum() > 0 and want[:, 1].sum() > 0
            if kind in ("ignore", "bg"):
                assert want[:, 2].sum() == 0


def test_head_metrics_adds_and_refuses(drn):
    """counts are ADDED to (two launches double them); outside the shape class DrnError, and nothing is launched for nh = 0 / M = 0"""
    from drn_wsod_pytorch_amd._cabi import DrnError

    rs = np.random.RandomState(5)
    x, used, col0s, ldl, labels = _case(rs, 70, 5, 2, "mixed")
    want = MU.head_counts(x, col0s, 5, labels, 70)
    xd = torch.from_numpy(x).to(DEV)
    lab = [torch.from_numpy(g).to(DEV) for g in labels]
    counts = torch.zeros((8, 8), dtype=torch.int32, device=DEV)
    drn.head_metrics(xd, col0s, 5, lab, 70, counts)
    drn.head_metrics(xd, col0s, 5, lab, 70, counts)
    assert np.array_equal(counts.cpu().numpy()[:2, :6], 2 * want)
    counts.zero_()
    drn.head_metrics(xd, [], 5, [], 70, counts)
    drn.head_metrics(xd, col0s, 5, lab, 0, counts)
    assert not counts.cpu().numpy().any()
    with pytest.raises(DrnError):
        drn.head_metrics(xd, [0] * 9, 5, lab * 5, 70, counts)  # nh > 8
    with pytest.raises(DrnError):
        drn.head_metrics(xd, [0], 1024, lab[:1], 70, counts)  # K + 1 > 1024
    with pytest.raises(DrnError):
        drn.head_metrics(xd, [ldl - 3], 5, lab[:1], 70, counts)  # columns outside the row


# ---------------------------------------------------------------------------------------------------- 2. drn_metrics_record
def _slot(host, s):
    return host[4 + s * W: 4 + (s + 1) * W].astype(np.int64) & 0xFFFFFFFF


def test_record_six_calls_on_four_slots(drn):
    r = drn.metrics_ring(4, DEV)
    script = [[0.5], [1.0, NAN, 2.0], [INF, 3.0], [-0.0, 1e-38, 7.0, 9.0], [2.5] * 16, [-INF, 4.0]]
    nhs = [0, 3, 8, 1, 2, 0]
    rs = np.random.RandomState(7)
    cnts, after, keep = [], [], []
    for i, (losses, nh) in enumerate(zip(script, nhs)):
        c = np.zeros((8, 8), dtype=np.int32)
        c[:nh, :6] = rs.randint(0, 5000, size=(nh, 6))
        cnts.append(c)
        r["counts"].copy_(torch.from_numpy(c))
        ts = [torch.tensor([v], dtype=torch.float32, device=DEV) for v in losses]
        keep.append(ts)
        drn.metrics_record(ts, r["counts"], nh, 100 + i, r["ring"], r["state"])
        after.append(r["counts"].clone())  # stream-ordered: no synchronisation between the calls
    host = r["buf"].cpu().numpy()
    assert host[:4].tolist() == [6, 0, 0, 0]
    for a in after:
        assert not a.cpu().numpy().any()  # the scratch is zero again after every call
    for i in (2, 3, 4, 5):
        rec = _slot(host, i % 4)
        assert rec[0] == i and rec[W - 1] == i and rec[1] == len(script[i]) and rec[2] == nhs[i] and rec[3] == 100 + i
        want = [MU.f32_bits(v) for v in script[i]] + [0] * (16 - len(script[i]))
        assert rec[4:20].tolist() == want, i  # the inputs' bit patterns: NaN, +-inf, -0 included
        assert rec[20:68].tolist() == cnts[i][:, :6].reshape(-1).tolist(), i
        assert rec[68:71].tolist() == [0, 0, 0]


def test_record_refuses_bad_arguments(drn):
    from drn_wsod_pytorch_amd._cabi import DrnError

    r = drn.metrics_ring(2, DEV)
    one = torch.ones(1, device=DEV)
    with pytest.raises(DrnError):
        drn.metrics_record([], r["counts"], 0, 1, r["ring"], r["state"])
    with pytest.raises(DrnError):
        drn.metrics_record([one] * 17, r["counts"], 0, 1, r["ring"], r["state"])
    with pytest.raises(DrnError):
        drn.metrics_record([one], r["counts"], 9, 1, r["ring"], r["state"])
    assert r["buf"].cpu().numpy().tolist() == [0] * (4 + 2 * W)


def test_pair_captured_and_replayed_with_changed_contents(drn):
    """head_metrics + metrics_record captured as a linear two-node graph; three replays with changed logits, labels and losses give
    three consecutive records with the changed values - the slot and every value come from device memory, nothing is frozen"""
    K, nh, M = 5, 2, 131
    rs = np.random.RandomState(11)
    x, used, col0s, ldl, labels = _case(rs, M, K, nh, "mixed")
    xd = torch.from_numpy(x).to(DEV)
    lab = torch.from_numpy(np.stack(labels)).to(DEV)
    losses = [torch.zeros(1, device=DEV) for _ in range(3)]
    r = drn.metrics_ring(4, DEV)

    def pair():
        drn.head_metrics(xd, col0s, K, lab, M, r["counts"])
        drn.metrics_record(losses, r["counts"], nh, M, r["ring"], r["state"])

    pair()  # record 0, eagerly
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        pair()
    want = []
    for step in range(3):
        x2, _, _, _, labels2 = _case(rs, M, K, nh, "mixed")
        xd.copy_(torch.from_numpy(x2))
        lab.copy_(torch.from_numpy(np.stack(labels2)))
        vals = [float(np.float32(rs.rand())) for _ in range(3)]
        for t, v in zip(losses, vals):
            t.fill_(v)
        g.replay()
        want.append((vals, MU.head_counts(x2, col0s, K, labels2, M)))
    host = r["buf"].cpu().numpy()
    assert host[0] == 4
    assert len({w[1].tobytes() for w in want}) == 3
    for i, (vals, counts) in enumerate(want, start=1):
        rec = _slot(host, i % 4)
        assert rec[0] == i and rec[W - 1] == i and rec[1] == 3 and rec[2] == nh and rec[3] == M
        assert rec[4:7].tolist() == [MU.f32_bits(v) for v in vals]
        assert rec[20: 20 + 6 * nh].tolist() == counts.reshape(-1).tolist()
    assert not r["counts"].cpu().numpy().any()


# ------------------------------------------------------------------------------------------------------- 3. through the model
def _batches(name):
    """three different batches of the fixture's images (+ spares): as they are, inverted with the objectness order flipped, mirrored"""
    load_package()
    d = G.load(name)
    ocfg = G.MODEL_CASES[name]
    base = G.batch_from(d)
    alt = [dict(b, image=(255.0 - b["image"]).contiguous(), objectness_logits=b["objectness_logits"].flip(0).contiguous())
           for b in base]
    alt2 = [dict(b, image=b["image"].flip(2).contiguous()) for b in base]
    bad = [dict(b) for b in alt]
    bad[0]["objectness_logits"] = bad[0]["objectness_logits"].clone()
    bad[0]["objectness_logits"][3] = NAN  # ONE NaN objectness logit: every loss of the step is NaN (tests/test_guard_gpu.py)
    mk = G.drn_inputs
    return ocfg, int(d["seed"]), dict(b0=mk(base), b1=mk(alt), b2=mk(alt2), bad=mk(bad), spare=mk(base),
                                      M=sum(len(b["objectness_logits"]) for b in base), n_img=len(base))


def _make(ocfg, seed, precision, M, nonfinite="off"):
    from drn_wsod_pytorch_amd.engine import build_optimizer

    cfg, model = G.drn_model(ocfg, seed, DEV, 5, precision)
    gen = torch.Generator().manual_seed(84)
    # dropout fixed by the dropout_masks hook: the same multipliers {0, 2} for every step and every run
    model.roi_heads.box_head.dropout_masks = [((torch.rand((M, dim), generator=gen) < 0.5).float() * 2.0).to(DEV)
                                              for dim in ocfg.dan_dim]
    model.train()
    return cfg, model, build_optimizer(cfg, model, nonfinite=nonfinite)


def _params(model, opt):
    eng = model.roi_heads._engine
    out = {"w": _i32(eng.arena_w).clone(), "m": _i32(opt._mom).clone()}
    for n, p in model.named_parameters():
        if p.requires_grad:
            out["p." + n] = _i32(p.detach().contiguous()).clone()
    return out


def _eager_run(name, precision, metrics_period, order=("b0", "b1", "b2"), nonfinite="off", B=None, ocfg=None, seed=None):
    """-> dict(losses per step as {name: bits}, params, records, per-step restated counts, names of the C calls made)"""
    from drn_wsod_pytorch_amd import _cabi
    from drn_wsod_pytorch_amd.engine import Trainer

    if B is None:
        ocfg, seed, B = _batches(name)
    cfg, model, opt = _make(ocfg, seed, precision, B["M"], nonfinite)
    seq = [B[k] for k in order] + [B["spare"], B["spare"]]
    tr = Trainer(cfg, model, iter(seq), optimizer=opt, start_iter=40, metrics_period=metrics_period, metrics_slots=8)
    calls, real = [], _cabi.call

    def spy(fn, *a):
        calls.append(fn)
        return real(fn, *a)

    _cabi.call = spy
    try:
        losses, restated, marks = [], [], []
        K = model.roi_heads.num_classes
        for _ in order:
            marks.append(len(calls))
            ld = tr.run_step()
            torch.cuda.synchronize()
            losses.append({k: MU.f32_bits(v.detach().cpu().numpy()) for k, v in ld.items()})
            st = model.roi_heads._last_state
            eng = model.roi_heads._engine
            col = {n: c for n, _, c, _ in eng.cols}
            tg = st["aux"]["targets"]
            pcl = getattr(model.roi_heads, "refine_mode", "oicr") == "pcl"
            col0s = [] if pcl else [col["r%d" % k] for k in range(len(tg))]
            restated.append(MU.head_counts(st["w"]["logits"].cpu().numpy(), col0s, K,
                                           [t["labels"].cpu().numpy() for t in tg], st["M"]))
        lost = tr.flush_metrics()
    finally:
        _cabi.call = real
    torch.cuda.synchronize()
    return dict(losses=losses, params=_params(model, opt), storage=tr.storage, lost=lost, restated=restated, calls=calls,
                last_step_calls=calls[marks[-1]:],
                M=B["M"], n_img=B["n_img"], trainer=tr)


@pytest.mark.parametrize("name,precision,nh", [("model_r50c4_tiny", "fp32", 3), ("model_r50c4_reg_tiny", "fp32", 4),
                                               ("model_wsddn_r50c4_tiny", "fp32", 0), ("model_r50c4_tiny", "bf16", 3)])
def test_eager_trainer_records_what_the_step_computed(name, precision, nh):
    on = _eager_run(name, precision, 2)   # drains behind steps 2 and (flush) 3
    off = _eager_run(name, precision, 0)
    # metrics on changes no loss bit and no parameter bit, and off issues neither launch
    assert on["losses"] == off["losses"]
    assert set(on["params"]) == set(off["params"])
    for k in on["params"]:
        assert torch.equal(on["params"][k], off["params"][k]), k
    assert "drn_head_metrics" not in off["calls"] and "drn_metrics_record" not in off["calls"]
    assert on["calls"].count("drn_metrics_record") == 3 and on["calls"].count("drn_head_metrics") == (3 if nh else 0)
    # every other launch of a step, in the same order (the last step: first-use self-checks are behind it in both runs)
    rest = [c for c in on["last_step_calls"] if c not in ("drn_head_metrics", "drn_metrics_record")]
    assert rest == off["last_step_calls"] and len(rest) > 10
    assert on["lost"] == 0 and off["trainer"].metrics is None
    st = on["storage"]
    assert on["restated"][0].shape == (nh, 6)
    for i in range(3):
        it = 40 + i
        for k, bits in on["losses"][i].items():
            h = dict((t, v) for v, t in st.history(k))
            assert MU.f32_bits(h[it]) == bits, (k, it)
        tot = 0.0
        for k in on["trainer"].metrics.names:
            tot = tot + float(np.array(on["losses"][i][k], dtype=np.uint32).view(np.float32))
        assert dict((t, v) for v, t in st.history("total_loss"))[it] == tot
        want = MU.scalars(on["restated"][i], on["M"], on["n_img"])
        assert len(want) >= 4 * nh
        for k, v in want.items():
            assert dict((t, x) for x, t in st.history(k))[it] == v, (k, it)
        if nh:
            c = on["restated"][i]
            assert (c[:, 0] + c[:, 1] + c[:, 2] == on["M"]).all() and c[:, 2].sum() > 0
    logged = {k for k in st._history if "_r" in k and ("fast_rcnn/" in k or "roi_head/" in k)}
    assert logged == set().union(*[set(MU.scalars(c, on["M"], on["n_img"])) for c in on["restated"]])
    assert list(on["trainer"].metrics.names) == list(on["losses"][0])


# ------------------------------------------------------------------------------------------------------------- 4. graphed step
def _graphed_run(metrics, sync_every_step, start_iter=100, steps=12):
    from drn_wsod_pytorch_amd.engine import GraphedTrainStep

    ocfg, seed, B = _batches("model_r50c4_tiny")
    cfg, model, opt = _make(ocfg, seed, "bf16", B["M"])
    ring = model.roi_heads.enable_metrics(slots=8) if metrics else None
    opt.enable_pipelined()
    seq = [B["b%d" % (i % 3)] for i in range(steps + 2)]
    stepper = GraphedTrainStep(model, opt, seq[0], start_iter=start_iter)
    assert stepper.metrics is ring
    read, recs, lost = [], [], 0
    for i in range(steps):
        losses = stepper.step(seq[i], seq[i + 1])
        if sync_every_step:
            torch.cuda.synchronize()
            read.append({k: MU.f32_bits(v.detach().cpu().numpy()) for k, v in losses.items()})
        if metrics and i + 1 in (6, 12):
            if i + 1 == 12:  # the first drain, six steps old
                r, l = ring.collect(wait=True)
                recs, lost = recs + r, lost + l
            ring.drain()
    if metrics:
        r, l = ring.collect(wait=True)  # waits for that one event
        recs, lost = recs + r, lost + l
    torch.cuda.synchronize()
    stepper.release()
    return read, recs, lost


def test_graphed_step_drained_without_a_sync_equals_a_run_that_reads_every_step():
    read, _, _ = _graphed_run(metrics=False, sync_every_step=True)
    _, recs, lost = _graphed_run(metrics=True, sync_every_step=False)
    assert lost == 0 and [it for it, _ in recs] == list(range(100, 112))
    assert len(read) == 12
    for (it, rec), want in zip(recs, read):
        assert {k: MU.f32_bits(rec[k]) for k in want} == want, it
        assert "fast_rcnn/cls_accuracy_r0" in rec and "roi_head/num_fg_samples_r2" in rec
    assert len({tuple(sorted(r.items())) for r in read}) > 1  # the steps differ


def test_graphed_full_step_records_every_replay():
    """GraphedFullStep (trainable trunk, FREEZE_AT = 2, fp32): five steps with metrics on, drained once at the end without reading
    any loss, equal the losses of a run without metrics that synchronises after every step; start_iter numbers the records.
    Deterministic mode: the trainable trunk's RoIPool backward otherwise accumulates with float atomics, and two runs differ in
    the last bits from the second step on, metrics or not."""
    from drn_wsod_pytorch_amd.engine import GraphedFullStep, build_optimizer

    pkg = load_package()
    pkg.set_deterministic(True)
    try:
        out = _full_step_runs(GraphedFullStep, build_optimizer)
    finally:
        pkg.set_deterministic(False)
    assert out["lost"] == 0 and [it for it, _ in out["recs"]] == [7, 8, 9, 10, 11]
    for (it, rec), want in zip(out["recs"], out["read"]):
        assert {k: MU.f32_bits(rec[k]) for k in want} == want, it
        assert "fast_rcnn/cls_accuracy_r2" in rec


def _full_step_runs(GraphedFullStep, build_optimizer):
    ocfg, seed, B = _batches("model_r50c4_tiny")
    seq = [B["b%d" % (i % 3)] for i in range(5)]
    out = {}
    for metrics in (False, True):
        cfg, model = G.drn_model(ocfg, seed, DEV, 2, "fp32")
        model.roi_heads.box_head.dropout_p = 0.0
        model.train()
        opt = build_optimizer(cfg, model)
        ring = model.roi_heads.enable_metrics(slots=8) if metrics else None
        stepper = GraphedFullStep(model, opt, seq[0], start_iter=7)
        assert stepper.metrics is ring
        read = []
        for b in seq:
            losses = stepper.step(b)
            if not metrics:
                torch.cuda.synchronize()
                read.append({k: MU.f32_bits(v.detach().cpu().numpy()) for k, v in losses.items()})
        if metrics:
            ring.drain()
            out["recs"], out["lost"] = ring.collect(wait=True)
        else:
            out["read"] = read
        torch.cuda.synchronize()
    return out


def test_enable_metrics_after_a_primed_graphed_step_is_refused():
    from drn_wsod_pytorch_amd._cabi import DrnError
    from drn_wsod_pytorch_amd.engine import GraphedTrainStep

    ocfg, seed, B = _batches("model_r50c4_tiny")
    cfg, model, opt = _make(ocfg, seed, "bf16", B["M"])
    opt.enable_pipelined()
    stepper = GraphedTrainStep(model, opt, B["b0"])
    model.roi_heads.enable_metrics(slots=4)  # not primed yet: fine
    model.roi_heads.disable_metrics()
    stepper.step(B["b0"], B["b1"])
    with pytest.raises(DrnError, match="after a graphed step was primed"):
        model.roi_heads.enable_metrics()
    stepper.release()
    assert model.roi_heads.enable_metrics(slots=4) is not None
    torch.cuda.synchronize()


# --------------------------------------------------------------------------------------------- 5. against the unmodified reference
def test_label_statistics_equal_the_reference():
    """tests/golden/metrics_r50c4_tiny.npz (gen_golden_metrics.py: the model_r50c4_tiny case rerun on the unmodified reference, its
    EventStorage read after each of the two steps; written only when every arg-max of the reference's logits has a relative margin
    >= 1e-3 over the runner-up - seed 32 has 8.2e-5 and is refused, the fixture holds seed 132 with its inputs).  The package's fp32 model, same weights, same two steps on the eager Trainer: every *_r{k} scalar
    the reference logged is equal (exact ratios of small integers: compared at 1e-12)."""
    from drn_wsod_pytorch_amd.engine import Trainer

    gold = G.load("metrics_r50c4_tiny")
    assert float(gold["min_margin"]) >= 1e-3
    ocfg = G.MODEL_CASES["model_r50c4_tiny"]
    cfg, model = G.drn_model(ocfg, int(gold["seed"]), DEV, 5, "fp32")
    model.roi_heads.box_head.dropout_p = 0.0  # the fixture was generated with dropout patched to identity
    model.train()
    batch = G.drn_inputs(G.batch_from(gold))
    steps = int(gold["steps"])
    tr = Trainer(cfg, model, iter([batch] * (steps + 2)), metrics_period=steps, metrics_slots=4)
    for _ in range(steps):
        tr.run_step()
    assert tr.flush_metrics() == 0
    keys = [str(k) for k in gold["names"]]
    assert len(keys) >= 4 * ocfg.refine_num  # at least the three sample counts and the accuracy of every branch
    for s in range(steps):
        vals = gold["step%d" % s]
        present = gold["present%d" % s]
        for k, v, p in zip(keys, vals, present):
            h = dict((t, x) for x, t in tr.storage._history.get(k, []))
            if not p:
                assert s not in h, (k, s)
                continue
            assert s in h, (k, s)
            assert abs(h[s] - float(v)) <= 1e-12, (k, s, h[s], float(v))


# ------------------------------------------------------------------------------------------------------------ 6. guard interplay
def test_a_step_the_guard_skips_is_still_recorded():
    ocfg, seed, B = _batches("model_wsddn_r50c4_tiny")
    order = ("b0", "bad", "b2")
    on = _eager_run(None, "bf16", 3, order, "skip", B, ocfg, seed)
    ctl = _eager_run(None, "bf16", 0, order, "skip", B, ocfg, seed)
    for k in on["params"]:
        assert torch.equal(on["params"][k], ctl["params"][k]), k
    assert not torch.isnan(on["params"]["w"].view(torch.float32)).any()
    tot = dict((t, v) for v, t in on["storage"].history("total_loss"))
    assert sorted(tot) == [40, 41, 42] and on["lost"] == 0
    assert np.isfinite(tot[40]) and np.isnan(tot[41]) and np.isfinite(tot[42])
    assert on["trainer"].check_finite()["bad"] == 1
