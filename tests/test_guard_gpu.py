"""The anomaly guard on the device (FusedSGD(nonfinite=...); detectron2/engine/train_loop.py:252-258 checks every iteration's summed
loss in front of the optimizer, so the reference's weights and momentum are always those of the last finite iteration):
  1. drn_loss_guard against a Python restatement over a scripted sequence of calls, both modes;
  2. the guarded flat / block updates: flag 0 = the unguarded entry point bit for bit, flag 1 = nothing moves;
  3. the guarded fused fc6 dW + SGD launches (plain and accumulating) at the shapes of test_gemm_tn_sgd_equals_unfused_pair;
  4. through the model, batches good, good, BAD, good on the eager plain step, the pipelined optimizer and GraphedTrainStep:
     "raise" keeps the state of the second step and names iteration 2, "skip" ends where a run without the bad batch ends
     (these FAIL without the guard: one NaN loss poisons every parameter);
  5. WSL.ITER_SIZE = 2, pipelined: a bad first micro-step drops its window, the next window matches the control run;
  6. all finite: guard "raise" against off, three graphed steps, every parameter torch.equal.
A batch is poisoned through its input alone: ONE NaN objectness logit.  It scales that proposal's pooled features (roi.hip: a
multiplier, no index), so the row's logits, every softmax over the proposals and the losses are NaN; the only index the heads derive
from scores is the OICR arg-max, which keeps its initial value on NaN comparisons and is clamped into the image's rows
(oicr_targets_body).  The PCL clustering and CSC kernels are not fed NaN here (their loops on NaN scores are unaudited)."""
import numpy as np
import pytest
import torch

import golden_util as G
from __graft_entry__ import load_package

pytestmark = pytest.mark.gpu
DEV = "cuda"
INF, NAN = float("inf"), float("nan")
SEG_DT = [("off", "<i8"), ("cnt", "<i8"), ("lr", "<f4"), ("wd", "<f4")]
RAISE, SKIP = 1, 2


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


def _flag(v):
    return torch.tensor([v, 0, -1, 0], dtype=torch.int32, device=DEV)


# ------------------------------------------------------------------------------------------------------------ 1. the check
# (losses, window_first): finite values, NaN, +-inf, inf + -inf, an overflowing sum of finite terms; 1 .. 7 losses
SCRIPT = [([0.5], 1), ([1.0, 2.0, 3.0, 0.25, 0.125, 7.0, 1e-3], 0), ([3e38, -3e38, 1.0], 1), ([1.0, NAN], 1), ([2.0, 3.0], 0),
          ([0.1, 0.2, 0.3, 0.4], 0), ([1.0], 1), ([INF, 1.0, 2.0, 3.0, 4.0], 0), ([1.0, 1.0], 0), ([-INF], 1), ([2.5] * 6, 1),
          ([INF, -INF], 1), ([1.0, 2.0], 1), ([3e38, 3e38], 0), ([3e38, 1e37], 0), ([1.0], 0), ([0.0], 1), ([NAN] * 7, 0),
          ([1.0, 2.0, 3.0], 1)]


def _restate(script, mode):
    """the rule of include/drn_wsod.h, in Python: fp32 sum in list order, isfinite(sum); raise = sticky, skip = per window"""
    flag, calls, first, bad, out = 0, 0, -1, 0, []
    with np.errstate(over="ignore", invalid="ignore"):
        for losses, wf in script:
            s = np.float32(0.0)
            for v in losses:
                s = np.float32(s + np.float32(v))
            b = not np.isfinite(s)
            keep = flag if mode == RAISE else (flag and not wf)
            flag = 1 if (b or keep) else 0
            if b:
                first = calls if first < 0 else first
                bad += 1
            calls += 1
            out.append([flag, calls, first, bad])
    return out


@pytest.mark.parametrize("mode", [RAISE, SKIP])
def test_loss_guard_follows_the_rule(drn, mode):
    ref = _restate(SCRIPT, mode)
    assert [r[0] for r in _restate(SCRIPT, SKIP)][:8] == [0, 0, 0, 1, 1, 1, 0, 1]  # (the script exercises both window rules)
    assert sorted({len(l) for l, _ in SCRIPT}) == [1, 2, 3, 4, 5, 6, 7]
    state = drn.loss_guard_state(DEV)
    assert state.tolist() == [0, 0, -1, 0]
    got = []
    for losses, wf in SCRIPT:
        ts = [torch.tensor([v], dtype=torch.float32, device=DEV) for v in losses]
        drn.loss_guard(ts, mode, wf, state)
        got.append(state.clone())  # stream-ordered: no synchronisation between the calls
    torch.cuda.synchronize()
    assert [g.tolist() for g in got] == ref
    assert ref[-1][3] == 6 and ref[-1][2] == 3  # bad: NaN, inf, -inf, inf + -inf, 3e38 + 3e38, NaN x 7


def test_loss_guard_refuses_bad_arguments(drn):
    from drn_wsod_pytorch_amd._cabi import DrnError

    state = drn.loss_guard_state(DEV)
    one = torch.ones(1, device=DEV)
    with pytest.raises(DrnError):
        drn.loss_guard([], RAISE, 1, state)
    with pytest.raises(DrnError):
        drn.loss_guard([one] * 17, RAISE, 1, state)
    with pytest.raises(DrnError):
        drn.loss_guard([one], 3, 1, state)
    drn.loss_guard([one] * 16, SKIP, 1, state)
    torch.cuda.synchronize()
    assert state.tolist() == [0, 1, -1, 0]


# ------------------------------------------------------------------------------------------- 2. flat and block updates
OFFS, LENS = [0, 1028, 2051], [1028, 1023, 517]  # the vector body, the scalar tail and an unaligned start are all hit


def _clip(drn, mode, grads, segs_dev, nseg, goff=0):
    if mode == 0:
        return None
    if mode == 1:
        return (drn.CLIP_VALUE, 0.5, None)
    return (drn.CLIP_NORM, 5.0, drn.grad_norms(grads, segs_dev, nseg, 2, 0.5, grad_off=goff))


@pytest.mark.parametrize("shadow", [False, True])
@pytest.mark.parametrize("gdt", [torch.float32, torch.bfloat16])
def test_guarded_flat_update(drn, gdt, shadow):
    """three segments of 1028 / 1023 / 517 elements at 0 / 1028 / 2051; clip modes 0 / 1 / 2 x first_step 0 / 1: with the flag clear
    the guarded entry point equals the unguarded one bit for bit, with the flag set weights / momentum / shadow keep their bits"""
    rs = np.random.RandomState(81)
    tot = OFFS[-1] + LENS[-1]
    segs = np.zeros(3, dtype=SEG_DT)
    for i in range(3):
        segs[i] = (OFFS[i], LENS[i], 0.01 * (i + 1), 5e-4 if i != 1 else 0.0)
    segs_dev = torch.from_numpy(segs.view(np.uint8)).to(DEV)
    w0 = torch.from_numpy(rs.standard_normal(tot).astype(np.float32)).to(DEV)
    m0 = torch.from_numpy(rs.standard_normal(tot).astype(np.float32)).to(DEV)
    s0 = w0.to(torch.bfloat16) if shadow else None
    g = torch.from_numpy(rs.standard_normal(tot).astype(np.float32)).to(DEV).to(gdt)
    for cm in (0, 1, 2):
        for first in (0, 1):
            clip = _clip(drn, cm, g, segs_dev, 3)
            ref = [w0.clone(), m0.clone(), s0.clone() if shadow else None]
            drn.sgd_step(ref[0], ref[1], g, segs_dev, 3, 0.9, first, 0.5, shadow=ref[2], clip=clip)
            for flag in (0, 1):
                got = [w0.clone(), m0.clone(), s0.clone() if shadow else None]
                drn.sgd_step(got[0], got[1], g, segs_dev, 3, 0.9, first, 0.5, shadow=got[2], clip=clip, guard=_flag(flag))
                want = ref if flag == 0 else [w0, m0, s0]
                for a, b in zip(got, want):
                    if a is not None:
                        assert torch.equal(_i32(a), _i32(b)), (cm, first, flag)
            assert not torch.equal(ref[0], w0)


@pytest.mark.parametrize("shadow", [False, True])
@pytest.mark.parametrize("gdt", [torch.float32, torch.bfloat16])
def test_guarded_block_update(drn, gdt, shadow):
    """the block form on the five-block partition of test_sgd_step_block_equals_flat (its shape class wants multiples of 4: one
    [70][1000] tensor at offset 192), same two assertions"""
    rs = np.random.RandomState(82)
    n0, rows, ld = 192, 70, 1000
    tot = n0 + rows * ld + 64
    seg = np.zeros(1, dtype=SEG_DT)
    seg[0] = (n0, rows * ld, 0.01, 5e-4)
    seg_dev = torch.from_numpy(seg.view(np.uint8)).to(DEV)
    w0 = torch.from_numpy(rs.standard_normal(tot).astype(np.float32)).to(DEV)
    m0 = torch.from_numpy(rs.standard_normal(tot).astype(np.float32)).to(DEV)
    s0 = w0.to(torch.bfloat16) if shadow else None
    g = torch.from_numpy(rs.standard_normal(rows * ld).astype(np.float32)).to(DEV).to(gdt)
    if gdt == torch.float32:
        ga, goff = torch.zeros_like(w0), 0
        ga[n0: n0 + rows * ld] = g
    else:
        ga, goff = g, n0
    blocks = [(0, rows, 768, 1000), (0, rows, 0, 256), (0, 32, 256, 768), (32, rows, 256, 512), (32, rows, 512, 768)]
    for cm in (0, 1, 2):
        for first in (0, 1):
            clip = _clip(drn, cm, ga, seg_dev, 1, goff)
            runs = {}
            for key in ("ref", 0, 1):
                st = [w0.clone(), m0.clone(), s0.clone() if shadow else None]
                for r0, r1, c0, c1 in blocks:
                    drn.sgd_step_block(st[0], st[1], ga, seg_dev, r0, r1 - r0, c0, c1 - c0, ld, 0.9, first, 0.5, shadow=st[2],
                                       grad_off=goff, clip=clip, guard=None if key == "ref" else _flag(key))
                runs[key] = st
            for a, b, c, d in zip(runs["ref"], runs[0], runs[1], [w0, m0, s0]):
                if a is not None:
                    assert torch.equal(_i32(a), _i32(b)), (cm, first)
                    assert torch.equal(_i32(c), _i32(d)), (cm, first)
            assert not torch.equal(runs["ref"][0], w0)


# --------------------------------------------------------------------------------------------------- 3. the fused launch
# the nine cases of tests/test_ops_gpu.py::test_gemm_tn_sgd_equals_unfused_pair (riding and exposed chunks)
FUSED = [(1024, 20480, 5e-4, 2048, 2000), (768, 24576 + 256, 0.0, 2048, 2000), (2048, 8192 + 512, 1e-4, 2048, 2048),
         (1024, 20480, 5e-4, 4032, 4000), (512, 40960 + 256, 1e-4, 2112, 2100), (1024, 20480, 5e-4, 1408, 1361),
         (768, 24576 + 256, 0.0, 576, 565), (1024, 20480, 5e-4, 1984, 1947), (512, 40960 + 256, 1e-4, 128, 100)]


@pytest.mark.parametrize("acc", [False, True])
@pytest.mark.parametrize("M,N,wd,K,kb", FUSED)
def test_guarded_fused_dw_sgd(drn, M, N, wd, K, kb, acc):
    """drn_gemm_tn_sgd_guard / drn_gemm_tn_acc_sgd_guard: flag 0 - bucket, weights, momentum, shadow torch.equal to the unguarded
    launch; flag 1 - weights / momentum / shadow equal to what they were as int views (the shadow holds bf16(weights), as every
    update leaves it), the bucket still written.  A first step and a momentum step."""
    gen = torch.Generator(device=DEV)
    gen.manual_seed(83)
    rnd = lambda *s: torch.randn(*s, generator=gen, device=DEV, dtype=torch.float32)
    seg = np.zeros(1, dtype=SEG_DT)
    seg[0] = (0, M * N, 0.01, wd)
    seg_dev = torch.from_numpy(seg.view(np.uint8)).to(DEV)
    w0 = rnd(M, N) * 0.02
    m0 = rnd(M, N) * 0.01
    s0 = w0.to(torch.bfloat16)
    A = torch.zeros((M, K), dtype=torch.bfloat16, device=DEV)
    A[:, :kb] = (rnd(M, kb) * 0.1).to(torch.bfloat16)
    Bt = (rnd(kb, N) * 0.1).to(torch.bfloat16)
    ga = rnd(M, N) * (0.01 * kb ** 0.5) if acc else None

    def run(w, m, s, first, guard):
        b = torch.full((M, N), 3.0, dtype=torch.bfloat16, device=DEV)
        if acc:
            assert drn.gemm_tn_acc_sgd(A, Bt, M, N, K, kb, ga, b, w, m, s, seg_dev, 0.9, first, 0.5, guard=guard)
        else:
            assert drn.gemm_tn_sgd(A, Bt, M, N, K, kb, b, w, m, s, seg_dev, 0.9, first, 0.5, guard=guard)
        return b

    for first in (1, 0):
        ref = [w0.clone(), m0.clone(), s0.clone()]
        bref = run(*ref, first, None)
        on = [w0.clone(), m0.clone(), s0.clone()]
        b0 = run(*on, first, _flag(0))
        off = [w0.clone(), m0.clone(), s0.clone()]
        b1 = run(*off, first, _flag(1))
        torch.cuda.synchronize()
        assert torch.equal(bref, b0) and torch.equal(bref, b1), first
        for a, b, c, d in zip(ref, on, off, [w0, m0, s0]):
            assert torch.equal(a, b), first
            assert torch.equal(_i32(c), _i32(d)), first
        assert not torch.equal(ref[0], w0) and not torch.equal(ref[1], m0)


# ------------------------------------------------------------------------------------------------- 4. through the model
def _batches(name):
    """single-image batches of the fixture: good, good', BAD (good with ONE NaN objectness logit), good'', and a spare"""
    load_package()
    d = G.load(name)
    ocfg = G.MODEL_CASES[name]
    base = G.batch_from(d)[0]
    alt = dict(base)
    alt["image"] = (255.0 - base["image"]).contiguous()
    alt["objectness_logits"] = base["objectness_logits"].flip(0).contiguous()
    alt2 = dict(base)
    alt2["image"] = base["image"].flip(2).contiguous()
    alt2["gt_classes"] = (base["gt_classes"] + 1) % ocfg.num_classes
    bad = dict(base)
    bad["objectness_logits"] = base["objectness_logits"].clone()
    bad["objectness_logits"][3] = NAN
    mk = lambda b: G.drn_inputs([b])
    return ocfg, int(d["seed"]), dict(good0=mk(base), good1=mk(alt), bad=mk(bad), good2=mk(alt2), spare=mk(base),
                                      M=len(base["objectness_logits"]))


def _make(ocfg, seed, nonfinite, precision, M, iter_size=1):
    from drn_wsod_pytorch_amd.engine import build_optimizer

    cfg, model = G.drn_model(ocfg, seed, DEV, 5, precision)
    cfg.WSL.ITER_SIZE = iter_size
    bh = model.roi_heads.box_head
    gen = torch.Generator().manual_seed(84)
    # dropout fixed by the dropout_masks hook: inverted-dropout multipliers {0, 2}, the same for every step and every run
    bh.dropout_masks = [((torch.rand((M, dim), generator=gen) < 0.5).float() * 2.0).to(DEV) for dim in ocfg.dan_dim]
    model.train()
    return cfg, model, build_optimizer(cfg, model, nonfinite=nonfinite)


def _state(model, opt):
    """every parameter, momentum and shadow element, as int views (NaN-proof equality)"""
    eng = model.roi_heads._engine
    out = {"w": _i32(eng.arena_w).clone(), "m": _i32(opt._mom).clone()}
    if eng.arena_s is not None:
        out["s"] = _i32(eng.arena_s).clone()
    for n, p in model.named_parameters():
        if p.requires_grad:
            out["p." + n] = _i32(p.detach().contiguous()).clone()
    return out


def _run(schedule, ocfg, seed, nonfinite, order, B, precision="bf16", snap_after=None):
    """`order`: batch names; returns (state after the run, state after step `snap_after`, check_finite's result or exception)"""
    from drn_wsod_pytorch_amd.engine import GraphedTrainStep, Trainer

    cfg, model, opt = _make(ocfg, seed, nonfinite, precision, B["M"])
    seq = [B[k] for k in order] + [B["spare"], B["spare"]]
    tr = Trainer(cfg, model, iter(seq), optimizer=opt)
    stepper, snap = None, None
    if schedule != "plain":
        opt.enable_pipelined()
    if schedule == "graphed":
        stepper = GraphedTrainStep(model, opt, seq[0])
    for i in range(len(order)):
        if stepper is not None:
            stepper.step(seq[i], seq[i + 1])
        else:
            tr.run_step()
        if snap_after == i:
            torch.cuda.synchronize()
            snap = _state(model, opt)
    torch.cuda.synchronize()
    end = _state(model, opt)
    if stepper is not None:
        stepper.release()
        tr.iter = len(order)  # (the Trainer did not drive these steps; its check reads the optimizer's guard all the same)
    try:
        res = tr.check_finite()
    except FloatingPointError as e:
        res = e
    return end, snap, res


ORDER = ["good0", "good1", "bad", "good2"]


@pytest.mark.parametrize("schedule", ["plain", "pipelined", "graphed"])
@pytest.mark.parametrize("name", ["model_wsddn_r50c4_tiny", "model_r50c4_tiny"])
def test_raise_keeps_the_last_finite_state(name, schedule):
    """good, good, BAD, good with nonfinite="raise": every parameter, momentum and shadow element equals the snapshot behind the
    second step, and check_finite() raises the reference's message naming iteration 2 (WSDDN and OICR heads)"""
    ocfg, seed, B = _batches(name)
    end, snap, res = _run(schedule, ocfg, seed, "raise", ORDER, B, snap_after=1)
    assert set(end) == set(snap) and "s" in end
    for k in end:
        assert torch.equal(end[k], snap[k]), k
    assert isinstance(res, FloatingPointError) and str(res) == "Loss became infinite or NaN at iteration=2!"


@pytest.mark.parametrize("schedule", ["plain", "pipelined", "graphed"])
def test_skip_equals_a_run_without_the_bad_batch(schedule):
    """nonfinite="skip" (constant LR): good, good, BAD, good ends bit for bit where good, good, good ends; the state reports one
    bad check, the third"""
    name = "model_wsddn_r50c4_tiny"
    ocfg, seed, B = _batches(name)
    end, _, res = _run(schedule, ocfg, seed, "skip", ORDER, B)
    ctl, _, res_ctl = _run(schedule, ocfg, seed, "skip", ["good0", "good1", "good2"], B)
    for k in end:
        assert torch.equal(end[k], ctl[k]), k
    assert (res["calls"], res["first_bad"], res["bad"], res["skip"], res["first_bad_iteration"]) == (4, 2, 1, False, 2)
    assert (res_ctl["calls"], res_ctl["first_bad"], res_ctl["bad"]) == (3, -1, 0)
    assert not torch.isnan(end["w"].view(torch.float32)).any()


def test_without_the_guard_one_bad_batch_poisons_the_run():
    """what the guard is for (and that the poisoned batch really is one): guard off, the same four batches leave NaN weights"""
    ocfg, seed, B = _batches("model_wsddn_r50c4_tiny")
    end, _, res = _run("pipelined", ocfg, seed, "off", ORDER, B)
    assert torch.isnan(end["w"].view(torch.float32)).any()
    assert isinstance(res, FloatingPointError)  # check_finite() as it was: the last losses, the current iteration
    assert str(res) == "Loss became infinite or NaN at iteration=4!"


# ------------------------------------------------------------------------------------------------ 5. accumulation windows
def test_skip_drops_the_whole_window_iter_size_2():
    """WSL.ITER_SIZE = 2 on the pipelined optimizer (windows {0}, {1, 2}, {3, 4}): iteration 1 - the FIRST micro-step of its window -
    is bad, the closing update behind iteration 2 is skipped, and the window {3, 4} ends where the control run's second window
    (the same two batches as its iterations 1, 2) ends"""
    from drn_wsod_pytorch_amd.engine import Trainer

    ocfg, seed, B = _batches("model_wsddn_r50c4_tiny")

    def run(order):
        cfg, model, opt = _make(ocfg, seed, "skip", "bf16", B["M"], iter_size=2)
        opt.enable_pipelined(iter_size=2)
        tr = Trainer(cfg, model, iter([B[k] for k in order] + [B["spare"], B["spare"]]), optimizer=opt)
        for _ in order:
            tr.run_step()
        torch.cuda.synchronize()
        return _state(model, opt), tr.check_finite()

    end, res = run(["good0", "bad", "good1", "good2", "good1"])
    ctl, res_ctl = run(["good0", "good2", "good1"])
    for k in end:
        assert torch.equal(end[k], ctl[k]), k
    assert (res["calls"], res["first_bad"], res["bad"], res["skip"]) == (5, 1, 1, False)
    assert res_ctl["bad"] == 0
    assert not torch.isnan(end["w"].view(torch.float32)).any()


# ---------------------------------------------------------------------------------------------------------- 6. all finite
def test_all_finite_guard_on_equals_guard_off_graphed():
    """three graphed steps of the tiny OICR model over finite batches: nonfinite="raise" and "off" give torch.equal parameters"""
    ocfg, seed, B = _batches("model_r50c4_tiny")
    order = ["good0", "good1", "good2"]
    on, _, res = _run("graphed", ocfg, seed, "raise", order, B)
    off, _, res_off = _run("graphed", ocfg, seed, "off", order, B)
    assert set(on) == set(off)
    for k in on:
        assert torch.equal(on[k], off[k]), k
    assert res["calls"] == 3 and res["bad"] == 0 and res_off is None
