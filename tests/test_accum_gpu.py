"""Gradient accumulation (WSL.ITER_SIZE = N > 1, projects/WSL/tools/train_net.py:100-113) on the pipelined optimizer and the
graphed step: the closing launch drn_gemm_tn_acc_sgd bit for bit against the sequence it fuses, the engine's window schedule with
the fused closing launch against the unfused one, the one bf16 rounding per window against the eager unpipelined Trainer, and the
graphed step in the fp32 parity mode against the eager loop with the reference's window rule."""
import numpy as np
import pytest
import torch

import golden_util as G
import resnet_std_util as U
from __graft_entry__ import load_package

pytestmark = pytest.mark.gpu
O = G.O
DEV = "cuda"


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


# the nine cases of tests/test_ops_gpu.py::test_gemm_tn_sgd_equals_unfused_pair
@pytest.mark.parametrize("M,N,wd,K,kb", [(1024, 20480, 5e-4, 2048, 2000), (768, 24576 + 256, 0.0, 2048, 2000),
                                         (2048, 8192 + 512, 1e-4, 2048, 2048), (1024, 20480, 5e-4, 4032, 4000),
                                         (512, 40960 + 256, 1e-4, 2112, 2100),
                                         (1024, 20480, 5e-4, 1408, 1361), (768, 24576 + 256, 0.0, 576, 565),
                                         (1024, 20480, 5e-4, 1984, 1947), (512, 40960 + 256, 1e-4, 128, 100)])
def test_gemm_tn_acc_sgd_equals_unfused_sequence(drn, M, N, wd, K, kb):
    """drn_gemm_tn_acc_sgd - G = bf16(grad_acc + A . Bt) and the optimizer step, one launch - against drn_gemm_tn (fp32 C,
    accumulate) on a copy of grad_acc, drn_cast2d to bf16, drn_sgd_step: bucket, weights, momentum and shadow bit for bit over
    three consecutive windows (a first step, then momentum), grad_acc untouched.  The accumulator holds seeded values of the
    products' magnitude (std 0.01 sqrt(kb)), so a sum formed in another association, or rounded twice, differs."""
    rs = np.random.RandomState(29)
    w0 = torch.from_numpy(rs.standard_normal((M, N)).astype(np.float32)).to(DEV) * 0.02
    seg = np.zeros(1, dtype=[("off", "<i8"), ("cnt", "<i8"), ("lr", "<f4"), ("wd", "<f4")])
    seg[0] = (0, M * N, 0.01, wd)
    seg_dev = torch.from_numpy(seg.view(np.uint8)).to(DEV)
    wa, ma, sa = w0.clone(), torch.zeros_like(w0), torch.zeros((M, N), dtype=torch.bfloat16, device=DEV)
    wb, mb, sb = w0.clone(), torch.zeros_like(w0), torch.zeros((M, N), dtype=torch.bfloat16, device=DEV)
    for step in range(3):
        A = torch.zeros((M, K), dtype=torch.bfloat16, device=DEV)
        A[:, :kb] = torch.from_numpy(rs.standard_normal((M, kb)).astype(np.float32)).to(DEV).to(torch.bfloat16) * 0.1
        Bt = (torch.from_numpy(rs.standard_normal((kb, N)).astype(np.float32)).to(DEV) * 0.1).to(torch.bfloat16)
        ld = N + (64 if step == 1 else 0)  # (a pitched accumulator once)
        full = torch.zeros((M, ld), dtype=torch.float32, device=DEV)
        acc0 = full[:, :N]
        acc0.copy_(torch.from_numpy(rs.standard_normal((M, N)).astype(np.float32)).to(DEV) * (0.01 * kb ** 0.5))
        # the unfused sequence
        ga = acc0.clone()
        drn.gemm_tn(A, Bt, M, N, K, kb, out=ga.unsqueeze(0), accumulate=True)
        g16 = torch.zeros((M, N), dtype=torch.bfloat16, device=DEV)
        drn.cast2d(ga, M, N, g16)
        drn.sgd_step(wa.view(-1), ma.view(-1), g16.view(-1), seg_dev, 1, 0.9, step == 0, 0.5, shadow=sa.view(-1))
        # the one launch
        keep = full.clone()
        gb = torch.full((M, N), 3.0, dtype=torch.bfloat16, device=DEV)
        assert drn.gemm_tn_acc_sgd(A, Bt, M, N, K, kb, acc0, gb, wb, mb, sb, seg_dev, 0.9, step == 0, 0.5)
        torch.cuda.synchronize()
        assert torch.equal(full, keep), step  # read, never written
        assert torch.equal(g16, gb), step
        assert torch.equal(wa, wb) and torch.equal(ma, mb) and torch.equal(sa, sb), step
        assert not torch.equal(g16, drn.gemm_tn(A, Bt, M, N, K, kb, out=torch.zeros((1, M, N), dtype=torch.bfloat16, device=DEV))[0])
    assert not torch.equal(wa, w0)
    # a zero accumulator: drn_gemm_tn_sgd's results, which this change must not move
    wc, mc, sc = wa.clone(), ma.clone(), sa.clone()
    wd_, md_, sd_ = wa.clone(), ma.clone(), sa.clone()
    gc, gd = torch.zeros_like(gb), torch.zeros_like(gb)
    assert drn.gemm_tn_sgd(A, Bt, M, N, K, kb, gc, wc, mc, sc, seg_dev, 0.9, False, 0.5)
    assert drn.gemm_tn_acc_sgd(A, Bt, M, N, K, kb, torch.zeros((M, N), dtype=torch.float32, device=DEV), gd, wd_, md_, sd_,
                               seg_dev, 0.9, False, 0.5)
    gr = torch.zeros((1, M, N), dtype=torch.bfloat16, device=DEV)
    drn.gemm_tn(A, Bt, M, N, K, kb, out=gr)
    drn.sgd_step(wa.view(-1), ma.view(-1), gr.view(-1), seg_dev, 1, 0.9, False, 0.5, shadow=sa.view(-1))
    torch.cuda.synchronize()
    assert torch.equal(gc, gr[0]) and torch.equal(wc, wa) and torch.equal(mc, ma) and torch.equal(sc, sa)
    assert torch.equal(gd, gc) and torch.equal(wd_, wc) and torch.equal(md_, mc) and torch.equal(sd_, sc)
    # outside the shape class nothing is launched
    before = (gb.clone(), wb.clone(), mb.clone(), sb.clone())
    if K >= 1088:  # (a contraction length that is not whole 64-element slabs)
        assert not drn.gemm_tn_acc_sgd(A[:, :1056].contiguous(), Bt[:1056].contiguous(), M, N, 1056, 1056, acc0, gb, wb, mb, sb,
                                       seg_dev, 0.9, False)
    odd = torch.zeros((M, N + 2), dtype=torch.float32, device=DEV)[:, :N]  # ld_acc % 4 != 0
    assert not drn.gemm_tn_acc_sgd(A, Bt, M, N, K, kb, odd, gb, wb, mb, sb, seg_dev, 0.9, False)
    torch.cuda.synchronize()
    for x, y in zip(before, (gb, wb, mb, sb)):
        assert torch.equal(x, y)
    # grad_acc == NULL is an argument error
    C = load_package()._cabi
    rc = C.lib().drn_gemm_tn_acc_sgd(C.ptr(A), C.ptr(Bt), None, C.ptr(gb), M, N, K, kb, K, N, N, N, C.ptr(wb), C.ptr(mb), C.ptr(sb),
                                     N, C.ptr(seg_dev), 0.9, 0, 1.0, C.stream())
    assert rc == -1


def _bench_shape_model(precision="bf16"):
    kw = dict(arch="wsr50", out_feature="res4", res5_dilation=1, num_classes=20)
    ocfg = O.OracleCfg(dropout=0.0, base_lr=2e-4, **kw)
    cfg, model = G.drn_model(ocfg, 3, "cuda", 5, precision)
    model.roi_heads.box_head.dropout_p = 0.0
    model.train()
    return ocfg, cfg, model


def _bench_shape_batch(R):
    kw = dict(arch="wsr50", out_feature="res4", res5_dilation=1, num_classes=20)
    ocfg = O.OracleCfg(dropout=0.0, base_lr=2e-4, **kw)
    b = O.synthetic_batch(1, R, ocfg, seed=79)
    return G.drn_inputs([dict(x, gt_boxes=torch.zeros(len(x["gt_classes"]), 4)) for x in b])


def _forever(batch):
    while True:
        yield batch


@pytest.mark.parametrize("R", [2000, 1361])
def test_engine_window_fused_closing_equals_unfused(R):
    """The bench shape in bf16, enable_pipelined(None, iter_size=4, fused_tn=True) against fused_tn=False over nine
    micro-iterations of the eager Trainer - windows {0}, {1..4}, {5..8}: weight, momentum and shadow arenas bit for bit; the
    fused closing launch runs on iterations 0, 4 and 8 only, and drn_gemm_tn_sgd never."""
    from drn_wsod_pytorch_amd import ops
    from drn_wsod_pytorch_amd.engine import Trainer, build_optimizer

    batch = _bench_shape_batch(R)
    res = []
    for fused in (False, True):
        _, cfg, model = _bench_shape_model()
        cfg.WSL.ITER_SIZE = 4
        opt = build_optimizer(cfg, model)
        opt.enable_pipelined(None, iter_size=4, fused_tn=fused)
        assert opt.iter_size == 4
        eng = model.roi_heads._engine
        tr = Trainer(cfg, model, _forever(batch), optimizer=opt)
        kinds = []
        for i in range(9):
            ops.GEMM_TIMING = []
            tr.run_step()
            torch.cuda.synchronize()
            kinds.append({t[3][0] for t in ops.GEMM_TIMING})
            ops.GEMM_TIMING = None
        assert opt._steps == 3
        for i, k in enumerate(kinds):
            assert "tn_sgd" not in k, i
            assert ("tn_acc_sgd" in k) == (fused and i % 4 == 0), (i, k)
        res.append(dict(w=eng.arena_w.clone(), m=opt._mom.clone(), s=eng.arena_s.clone()))
        del model, opt, tr
        torch.cuda.empty_cache()
    for k in ("w", "m", "s"):
        assert torch.equal(res[0][k], res[1][k]), k


def test_one_rounding_per_window_bounded_against_eager_trainer():
    """bf16, the window {1..4} from a fresh optimizer (start_iter = 1: a first step, no momentum history).  The eager UNPIPELINED
    Trainer with ITER_SIZE 4 accumulates the same fp32 G in its gradient arena (same kernels, same order): asserted against the
    accumulator of the unfused fast path bit for bit, and against the fused path's bucket = bf16(G).  The fast path rounds G to
    bf16 once, so per element of fc1.weight
        |w_fast - w_eager| <= lr * 2^-8 * |G * grad_scale| + 2^-22 * |w|
    (unit round-off of one bf16 rounding times the step; four fp32 operations' worth of rounding).  The small tensors never pass
    through bf16: bit-equal."""
    from drn_wsod_pytorch_amd.engine import Trainer, build_optimizer

    batch = _bench_shape_batch(2000)
    out = {}
    for mode in ("eager", "fused", "unfused"):
        _, cfg, model = _bench_shape_model()
        cfg.WSL.ITER_SIZE = 4
        opt = build_optimizer(cfg, model)
        if mode != "eager":
            opt.enable_pipelined(None, iter_size=4, fused_tn=(mode == "fused"))
        eng = model.roi_heads._engine
        w0 = eng.arena_w.clone() if mode == "eager" else None
        tr = Trainer(cfg, model, _forever(batch), optimizer=opt, start_iter=1)
        for i in range(4):
            tr.run_step()
        torch.cuda.synchronize()
        assert opt._steps == 1
        o, n = eng._seg["fc1.weight"]
        lr = [g["lr"] for g in opt.param_groups if g["name"] == "fc1.weight"][0]
        out[mode] = dict(w=eng.arena_w.clone(), G=eng.arena_g[o: o + n].clone(), o=o, n=n, lr=lr, w0=w0,
                         bucket=None if mode == "eager" else eng.fc1_grad_bucket.clone().view(-1))
        del model, opt, tr
        torch.cuda.empty_cache()
    e, f, u = out["eager"], out["fused"], out["unfused"]
    o, n, lr = e["o"], e["n"], e["lr"]
    assert torch.equal(u["G"], e["G"])                       # the same fp32 sum, bit for bit
    assert torch.equal(u["bucket"], e["G"].to(torch.bfloat16))  # rounded once (round to nearest even)
    assert torch.equal(f["bucket"], u["bucket"])
    assert torch.equal(f["w"], u["w"])
    assert float(e["G"].abs().max()) > 0
    grad_scale = 1.0
    wf, we = f["w"][o: o + n].double(), e["w"][o: o + n].double()
    bound = lr * 2.0 ** -8 * (e["G"].double() * grad_scale).abs() + 2.0 ** -22 * we.abs()
    diff = (wf - we).abs()
    worst = float((diff - bound).max())
    print("fc1.weight: max |w_fast - w_eager| %.3e, max bound %.3e, max (diff - bound) %.3e, moved by %.3e"
          % (float(diff.max()), float(bound.max()), worst, float((we - e["w0"][o: o + n].double()).abs().max())))
    assert worst <= 0.0
    assert not torch.equal(e["w"][o: o + n], e["w0"][o: o + n])
    assert torch.equal(f["w"][:o], e["w"][:o])  # small tensors


def _three_batches(d, num_classes):
    """three different single-image batches of one shape (tests/test_model_gpu.py::test_hipgraph_step_equals_eager)"""
    base = G.batch_from(d)
    alt = dict(base[0])
    alt["image"] = (255.0 - base[0]["image"]).contiguous()
    alt["objectness_logits"] = base[0]["objectness_logits"].flip(0).contiguous()
    alt2 = dict(base[0])
    alt2["image"] = base[0]["image"].flip(2).contiguous()
    alt2["proposal_boxes"] = base[0]["proposal_boxes"].flip(0).contiguous()
    alt2["gt_classes"] = (base[0]["gt_classes"] + 1) % num_classes
    return [G.drn_inputs([b]) for b in (base[0], alt, alt2)]


def _tiny_fp32(name, tmp_path):
    """(cfg, model, the non-periodic batch sequence) of a tiny fixture in the fp32 parity mode, dropout off"""
    d = G.load(name)
    if name == "model_r50std_tiny":
        from drn_wsod_pytorch_amd.modeling import build_model

        load_package().set_precision("fp32")
        opts = [str(o) for o in d["cfg_opts"]]
        cfg = U.recorded_cfg(opts[0], tmp_path, opts[1:] + ["SOLVER.BASE_LR", "0.0002"], DEV)
        model = build_model(cfg)
        sd = model.state_dict()
        model.load_state_dict({n: (t if n in ("pixel_mean", "pixel_std") else O.seeded_tensor(n, tuple(t.shape), 71))
                               for n, t in sd.items()})
        K = 5
    else:
        ocfg = G.MODEL_CASES[name]
        cfg, model = G.drn_model(ocfg, int(d["seed"]), "cuda", 5, "fp32")
        K = ocfg.num_classes
    model.roi_heads.box_head.dropout_p = 0.0
    model.train()
    b0, b1, b2 = _three_batches(d, K)
    seq = [b0, b1, b2, b0, b1, b1, b0, b2, b1, b0, b2, b2, b0, b1, b0, b2]  # not periodic in 2, 3 or 4
    return cfg, model, seq


def _eager_window_loop(model, opt, seq, N, first, last):
    """the reference's loop (train_net.py:100-113) on the plain optimizer: loss / N, step + zero_grad when it % N == 0"""
    out = []
    opt.zero_grad()
    for i in range(first, last + 1):
        losses = model(seq[i])
        (sum(losses.values()) / N).backward()
        if i % N == 0:
            opt.step()
            opt.zero_grad()
        out.append({k: float(v.detach()) for k, v in losses.items()})
    torch.cuda.synchronize()
    return out


def _params(model):
    return {n: p.detach().clone() for n, p in model.named_parameters() if p.requires_grad}


def _assert_params_close(pe, pg):
    # fp32 parity, the same kernels in another schedule: the relative bound test_hipgraph_step_equals_eager puts on the losses,
    # per tensor against its largest element
    assert sorted(pe) == sorted(pg) and len(pe) > 0
    for n in pe:
        tol = 1e-5 * max(float(pe[n].abs().max()), 1e-3)
        assert float((pe[n] - pg[n]).abs().max()) <= tol, (n, float((pe[n] - pg[n]).abs().max()), tol)


@pytest.mark.parametrize("schedule", ["ring_group2", "lookahead1"])
@pytest.mark.parametrize("name", ["model_r50c4_tiny", "model_r50std_tiny"])
def test_graphed_step_accumulates_like_the_eager_loop(name, schedule, tmp_path):
    """fp32 parity: GraphedTrainStep with iter_size = 4 (OICR heads; the WSDDN head of the plain-ResNet recipes, the family
    that ships ITER_SIZE 32) over nine micro-iterations of a batch sequence that is not periodic, against the eager unpipelined
    loop with the reference's window rule: every loss within 1e-5 relative, the trainable parameters after iteration 8 close."""
    from drn_wsod_pytorch_amd.engine import GraphedTrainStep, build_optimizer

    N, steps = 4, 9
    cfg, model, seq = _tiny_fp32(name, tmp_path)
    opt = build_optimizer(cfg, model)
    eager = _eager_window_loop(model, opt, seq, N, 0, steps - 1)
    assert opt._steps == 3
    pe = _params(model)
    del model, opt
    cfg, model, seq = _tiny_fp32(name, tmp_path)
    opt = build_optimizer(cfg, model)
    opt.enable_pipelined(None, iter_size=N)
    if schedule == "ring_group2":
        stepper = GraphedTrainStep(model, opt, seq[0], split_tail=True, trunk_pairs=True, ring=True)
        width = 4
    else:
        stepper = GraphedTrainStep(model, opt, seq[0], ring=False, lookahead=1)
        width = 3
    got = []
    for i in range(steps):
        losses = stepper.step(*seq[i: i + width])
        got.append({k: float(v.detach()) for k, v in losses.items()})
    torch.cuda.synchronize()
    if schedule == "ring_group2":
        assert stepper._ring_on
    assert opt._steps == 3
    for i, (e, g) in enumerate(zip(eager, got)):
        print(name, schedule, i, e, g)
    for i, (e, g) in enumerate(zip(eager, got)):
        assert sorted(e) == sorted(g)
        for k in e:
            assert abs(e[k] - g[k]) <= 1e-5 * max(abs(e[k]), 1e-3), (i, k, e[k], g[k])
    _assert_params_close(pe, _params(model))
    stepper.release()


def test_graphed_step_window_alignment_on_resume(tmp_path):
    """start_iter = 7, N = 4: iteration 7 only accumulates, the first optimizer step is behind iteration 8 (8 % 4 == 0), and the
    parameters are the eager loop's."""
    from drn_wsod_pytorch_amd.engine import GraphedTrainStep, build_optimizer

    N = 4
    cfg, model, seq = _tiny_fp32("model_r50c4_tiny", tmp_path)
    opt = build_optimizer(cfg, model)
    _eager_window_loop(model, opt, seq, N, 7, 8)
    assert opt._steps == 1
    pe = _params(model)
    del model, opt
    cfg, model, seq = _tiny_fp32("model_r50c4_tiny", tmp_path)
    p0 = _params(model)
    opt = build_optimizer(cfg, model)
    opt.enable_pipelined(None, iter_size=N)
    stepper = GraphedTrainStep(model, opt, seq[7], ring=False, lookahead=1, start_iter=7)
    stepper.step(*seq[7: 10])
    torch.cuda.synchronize()
    assert opt._steps == 0
    for n, p in _params(model).items():
        assert torch.equal(p, p0[n]), n  # nothing moved yet
    stepper.step(*seq[8: 11])
    torch.cuda.synchronize()
    assert opt._steps == 1
    _assert_params_close(pe, _params(model))
    stepper.step(*seq[9: 12])  # iteration 9 opens the next window: accumulates only
    torch.cuda.synchronize()
    assert opt._steps == 1
    stepper.release()
