"""Trainer-side behaviour on the device (engine.py):
  * save -> resume -> continue equals uninterrupted training, optimizer momentum + LR schedule + iteration included
    (DefaultTrainer.resume_or_load, detectron2/engine/defaults.py:304-319);
  * a graphed step whose SGD launches are INSIDE the captured graph follows scheduler.step() between replays;
  * two ranks with WSL.ITER_SIZE = 2 (DDP no_sync for the non-final micro-steps) equal single-process training on the
    mean gradient (projects/WSL/tools/train_net.py:100-113 + detectron2/engine/defaults.py:279-282)."""
import itertools
import os
import socket

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

import golden_util as G
from __graft_entry__ import load_package

pytestmark = pytest.mark.gpu
load_package()
NAME = "model_r50c4_tiny"


def _three_batches():
    d = G.load(NAME)
    ocfg = G.MODEL_CASES[NAME]
    base = G.batch_from(d)
    alt = dict(base[0])
    alt["image"] = (255.0 - base[0]["image"]).contiguous()
    alt["objectness_logits"] = base[0]["objectness_logits"].flip(0).contiguous()
    alt2 = dict(base[0])
    alt2["image"] = base[0]["image"].flip(2).contiguous()
    alt2["proposal_boxes"] = base[0]["proposal_boxes"].flip(0).contiguous()
    alt2["gt_classes"] = (base[0]["gt_classes"] + 1) % ocfg.num_classes
    return int(d["seed"]), ocfg, [G.drn_inputs([base[0]]), G.drn_inputs([alt]), G.drn_inputs([alt2])]


def _model(seed, ocfg, iter_size=1):
    cfg, model = G.drn_model(ocfg, seed, "cuda", 5, "fp32")
    cfg.WSL.ITER_SIZE = iter_size
    model.roi_heads.box_head.dropout_p = 0.0
    model.train()
    return cfg, model


def _weights(model):
    return {n: p.detach().cpu().numpy().copy() for n, p in model.named_parameters() if p.requires_grad}


def test_save_resume_continue_equals_uninterrupted(tmp_path):
    from drn_wsod_pytorch_amd.checkpoint import DetectionCheckpointer
    from drn_wsod_pytorch_amd.engine import Trainer, WarmupMultiStepLR, build_optimizer

    seed, ocfg, batches = _three_batches()
    order = [0, 1, 2, 1, 0, 2, 2, 1, 0]

    def stream(start):
        return iter([batches[i] for i in order[start:]] + [batches[0]] * 4)

    def make(start_iter=0):
        cfg, model = _model(seed, ocfg)
        opt = build_optimizer(cfg, model)
        sched = WarmupMultiStepLR(opt, [3], gamma=0.5, warmup_factor=0.1, warmup_iters=2)
        return cfg, model, opt, sched

    # uninterrupted: 5 iterations
    cfg, model, opt, sched = make()
    tr = Trainer(cfg, model, stream(0), optimizer=opt, scheduler=sched)
    for _ in range(5):
        tr.run_step()
    torch.cuda.synchronize()
    want = _weights(model)
    want_lr = [g["lr"] for g in opt.param_groups]
    # interrupted after 3 iterations
    cfg, model, opt, sched = make()
    tr = Trainer(cfg, model, stream(0), optimizer=opt, scheduler=sched)
    for _ in range(3):
        tr.run_step()
    ck = DetectionCheckpointer(model, str(tmp_path), optimizer=opt, scheduler=sched)
    ck.save("model_0000002", iteration=tr.iter - 1)
    del tr, model, opt, sched
    # a fresh process would build everything anew and resume
    cfg, model, opt, sched = make()
    ck = DetectionCheckpointer(model, str(tmp_path), optimizer=opt, scheduler=sched)
    tr = Trainer(cfg, model, stream(3), optimizer=opt, scheduler=sched)
    tr.resume_or_load(ck, "", resume=True)
    assert tr.iter == 3 and tr.start_iter == 3 and sched.last_epoch == 3 and opt._steps == 3
    assert opt._mom.is_cuda and opt._mom.data_ptr() != 0
    for _ in range(2):
        tr.run_step()
    torch.cuda.synchronize()
    got = _weights(model)
    assert [g["lr"] for g in opt.param_groups] == want_lr
    for n in want:
        assert np.array_equal(got[n], want[n]), n  # same kernels, same inputs, restored state: bit-identical


def test_graphed_step_with_captured_sgd_follows_the_lr_schedule():
    from drn_wsod_pytorch_amd.engine import GraphedTrainStep, WarmupMultiStepLR, build_optimizer

    seed, ocfg, batches = _three_batches()
    seq = [batches[i] for i in (0, 1, 2, 0, 1, 1, 0, 2, 1, 0)]
    res = []
    for graphed in (False, True):
        cfg, model = _model(seed, ocfg)
        opt = build_optimizer(cfg, model)
        sched = WarmupMultiStepLR(opt, [2, 4], gamma=0.1, warmup_factor=0.01, warmup_iters=2)
        if graphed:
            stepper = GraphedTrainStep(model, opt, seq[0], split_tail=False)  # optimizer.step() inside the captured graph
        for i in range(6):
            if graphed:
                stepper.step(seq[i], seq[i + 1])
            else:
                opt.zero_grad()
                sum(model(seq[i]).values()).backward()
                opt.step()
            sched.step()  # warm-up then two decays: the LR differs on every one of the six steps
        torch.cuda.synchronize()
        res.append(_weights(model))
    for n in res[0]:
        a, b = res[0][n], res[1][n]
        assert np.abs(a - b).max() <= 1e-6 * max(np.abs(a).max(), 1e-3), n


# ------------------------------------------------------------------------------------------------------------------
def _worker(rank, world, port, q):
    try:
        os.environ["MASTER_ADDR"], os.environ["MASTER_PORT"] = "127.0.0.1", str(port)
        torch.cuda.set_device(0)
        dist.init_process_group("gloo", rank=rank, world_size=world)
        load_package()
        from drn_wsod_pytorch_amd.engine import DataParallel, Trainer, build_optimizer

        seed, ocfg, batches = _three_batches()
        cfg, model = _model(seed + 10 * rank, ocfg, iter_size=2)  # ranks start different: the broadcast fixes it
        opt = build_optimizer(cfg, model)
        dp = DataParallel(model)
        dp.broadcast_parameters(0)
        mine = [batches[(rank + j) % 3] for j in range(8)]
        tr = Trainer(cfg, model, iter(mine), optimizer=opt, parallel=dp)
        for _ in range(5):  # optimizer steps at iterations 0, 2, 4 (train_net.py:105); windows {0}, {1,2}, {3,4}
            tr.run_step()
        torch.cuda.synchronize()
        q.put((rank, "ok", _weights(model)))
    except Exception as ex:  # noqa: BLE001
        import traceback

        q.put((rank, "FAIL: %r\n%s" % (ex, traceback.format_exc()), None))
    finally:
        if dist.is_initialized():
            dist.destroy_process_group()


def test_two_ranks_iter_size_two_equals_mean_gradient_training():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    res = sorted([q.get(timeout=600) for _ in procs], key=lambda t: t[0])
    for p in procs:
        p.join(timeout=60)
    for r in res:
        assert r[1] == "ok", r[1]
    for n in res[0][2]:
        assert np.array_equal(res[0][2][n], res[1][2][n]), n  # replicas stay identical
    # single process on the mean gradient: per window, every rank's micro-batches at weight 1/ITER_SIZE * 1/world
    from drn_wsod_pytorch_amd.engine import build_optimizer

    seed, ocfg, batches = _three_batches()
    cfg, model = _model(seed, ocfg)
    opt = build_optimizer(cfg, model)
    per_rank = [[batches[(rank + j) % 3] for j in range(8)] for rank in range(2)]
    for window in ([0], [1, 2], [3, 4]):
        opt.zero_grad()
        for it, rank in itertools.product(window, range(2)):
            (sum(model(per_rank[rank][it]).values()) * 0.25).backward()
        opt.step()
    torch.cuda.synchronize()
    for n, p in model.named_parameters():
        if p.requires_grad and n in res[0][2]:
            diff = float((p.detach().cpu() - torch.from_numpy(res[0][2][n])).abs().max())
            # ((a + b) / 2 + (c + d) / 2 vs (a + b + c + d) / 4 in fp32, through three optimizer steps: 1e-6 .. 1.2e-5 measured)
            assert diff <= 3e-5 * max(float(p.detach().abs().max()), 1.0), (n, diff)


@pytest.mark.parametrize("name,freeze_at", [("model_r50c4_tiny", 2), ("model_r50c4_align_tiny", 3), ("model_r18dc5_tiny", 1)])
def test_graphed_full_step_trainable_trunk_equals_eager(name, freeze_at):
    """MODEL.BACKBONE.FREEZE_AT < 5 as one hipGraph (GraphedFullStep): trunk forward with saved activations, heads,
    explicit backward down to the first trainable block, SGD of both arenas and the re-pack of the updated conv weights
    - six steps over three batches must reproduce the eager trainer (losses and every trainable tensor)."""
    from drn_wsod_pytorch_amd.engine import GraphedFullStep, GraphedTrainStep, build_optimizer
    from drn_wsod_pytorch_amd._cabi import DrnError

    d = G.load(name)
    ocfg = G.MODEL_CASES[name]
    base = G.batch_from(d)
    alt = dict(base[0])
    alt["image"] = (255.0 - base[0]["image"]).contiguous()
    alt["objectness_logits"] = base[0]["objectness_logits"].flip(0).contiguous()
    alt2 = dict(base[0])
    alt2["image"] = base[0]["image"].flip(2).contiguous()
    alt2["gt_classes"] = (base[0]["gt_classes"] + 1) % ocfg.num_classes
    bs = [G.drn_inputs([base[0]]), G.drn_inputs([alt]), G.drn_inputs([alt2])]
    seq = [bs[i] for i in (0, 1, 2, 1, 0, 2)]
    res = []
    for graphed in (False, True):
        cfg, model = G.drn_model(ocfg, int(d["seed"]), "cuda", freeze_at, "fp32")
        model.roi_heads.box_head.dropout_p = 0.0
        model.train()
        opt = build_optimizer(cfg, model)
        assert any(n.startswith("backbone.") for n, p in model.named_parameters() if p.requires_grad)
        out = []
        if graphed:
            with pytest.raises(DrnError):
                GraphedTrainStep(model, opt, seq[0])  # the frozen-trunk schedule refuses a trainable trunk, loudly
            stepper = GraphedFullStep(model, opt, seq[0])
        for b in seq:
            if graphed:
                losses = stepper.step(b)
            else:
                opt.zero_grad()
                losses = model(b)
                sum(losses.values()).backward()
                opt.step()
            out.append({k: float(v.detach()) for k, v in losses.items()})
        torch.cuda.synchronize()
        res.append((out, _weights(model)))
    # RoIPool / ROIAlign backward scatters with float atomics, so two runs of the SAME trainable-trunk step differ in the
    # last bits of the trunk gradients, and over six steps a pooled arg-max or a ReLU flips in some runs: measured
    # run-to-run (eager vs eager, tools: six steps, this fixture) up to 4e-3 of a tensor's scale on the weights and
    # 1.4e-3 on the losses, bimodal.  The comparison below is therefore statistical (3x that floor); the failure modes
    # that are NOT noise are checked exactly: the graphed step must have re-packed every trainable conv from its updated
    # weights (a stale pack = the trunk silently stops learning in the forward), and must have touched every tensor.
    for e, g in zip(res[0][0], res[1][0]):
        for k in e:
            assert abs(e[k] - g[k]) <= 5e-3 * max(abs(e[k]), 1e-2), (k, e[k], g[k])
    for n in res[0][1]:
        a, b = res[0][1][n], res[1][1][n]
        assert np.abs(a - b).max() <= 1.2e-2 * max(np.abs(a).max(), 1e-3), n
    before = {n: t.numpy() for n, t in G.drn_model(ocfg, int(d["seed"]), "cpu", freeze_at, "fp32")[1].state_dict().items()}
    for n, b in res[1][1].items():  # every tensor the eager run moved moved under the graph (bbox_pred of non-regressing
        assert np.array_equal(b, before[n]) == np.array_equal(res[0][1][n], before[n]), n  # branches is unused in both)
    from drn_wsod_pytorch_amd.layers import Conv2d

    convs = [m for m in model.backbone.modules() if isinstance(m, Conv2d) and m.weight.requires_grad]  # the graphed run's
    assert convs
    w6 = [m.weight.detach().clone() for m in convs]
    stepper.step(seq[0])  # a seventh replay: its forward starts by packing the weights the sixth step left behind
    torch.cuda.synchronize()
    for m, w in zip(convs, w6):
        held = m._pack[0].clone()
        assert not torch.equal(m.weight.detach(), w)  # (the seventh update has happened in the meantime)
        with torch.no_grad():
            m.weight.copy_(w)
        m.invalidate_packs()
        assert torch.equal(held, m.packed(torch.float32)[0])


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_workspace_views_follow_changing_proposal_counts(precision):
    """Real data brings another proposal count every step.  The head engine's workspaces and fc6-operand sets are
    capacity-based views (head_engine.py `_HeadEngine.ws` / `pool`): after a LARGER batch the buffers still hold that
    batch's values beyond the new M - the K-role pad columns of the transposed twins (read by the dW GEMMs) must be
    zero again.  Losses and every gradient of [large, then small] must equal BIT FOR BIT those of a fresh model that
    only ever saw the small batch (M = 37: pad up to 64 in bf16, to 40 in fp32)."""
    from drn_wsod_pytorch_amd.engine import build_optimizer

    d = G.load(NAME)
    ocfg = G.MODEL_CASES[NAME]
    base = G.batch_from(d)[0]
    big = dict(base)
    jit = torch.linspace(0.0, 3.0, 3).view(3, 1, 1)
    big["proposal_boxes"] = (base["proposal_boxes"].unsqueeze(0) + jit).reshape(-1, 4).contiguous()
    big["objectness_logits"] = base["objectness_logits"].repeat(3).contiguous()
    small = dict(base)
    small["proposal_boxes"] = base["proposal_boxes"][:37].contiguous()
    small["objectness_logits"] = base["objectness_logits"][:37].contiguous()
    seed = int(d["seed"])

    def run(seq):
        cfg, model = G.drn_model(ocfg, seed, "cuda", 5, precision)
        model.roi_heads.box_head.dropout_p = 0.0
        model.train()
        opt = build_optimizer(cfg, model)
        for b in seq:
            opt.zero_grad()
            losses = model(G.drn_inputs([b]))
            sum(losses.values()).backward()
        torch.cuda.synchronize()
        return ({k: float(v.detach()) for k, v in losses.items()},
                {n: p.grad.detach().cpu().clone() for n, p in model.named_parameters() if p.grad is not None})

    l_seq, g_seq = run([big, small])
    l_one, g_one = run([small])
    assert l_seq == l_one
    assert set(g_seq) == set(g_one) and len(g_one) >= 6
    for n in g_one:
        assert torch.equal(g_seq[n], g_one[n]), n
    # and growing again after the small batch reproduces the large one
    l_big2, g_big2 = run([small, big])
    l_big1, g_big1 = run([big])
    assert l_big2 == l_big1
    for n in g_big1:
        assert torch.equal(g_big2[n], g_big1[n]), n


def test_backward_losses_equals_autograd():
    """GeneralizedRCNNWSL.backward_losses(scale) - the explicit backward called directly, what Trainer.run_step uses -
    against (scale * sum(loss_dict.values())).backward() (projects/WSL/tools/train_net.py:100-107): every gradient
    bit-equal, for scale 1 and for 1 / ITER_SIZE."""
    from drn_wsod_pytorch_amd.engine import build_optimizer

    seed, ocfg, batches = _three_batches()

    def grads(direct, scale):
        cfg, model = _model(seed, ocfg)
        opt = build_optimizer(cfg, model)
        opt.zero_grad()
        losses = model(batches[0])
        if direct:
            assert model.backward_losses(scale)
        else:
            (sum(losses.values()) * scale).backward()
        torch.cuda.synchronize()
        return {n: p.grad.detach().cpu().clone() for n, p in model.named_parameters() if p.grad is not None}

    for scale in (1.0, 0.25):
        a, b = grads(True, scale), grads(False, scale)
        assert set(a) == set(b) and len(a) >= 6
        for n in a:
            assert torch.equal(a[n], b[n]), (n, scale)


def test_dropout_counter_advances_without_its_own_launch():
    """The counter-based dropout masks are keyed by a device-side counter that the heads' logits pass advances behind the
    two dropout layers (drn_bias_act_fwd without dropout + seed_dev: *seed_dev += seed).  Two training forwards of the
    same batch with the same weights must therefore draw different masks (different losses), and rewinding the counter
    must reproduce the first draw bit for bit."""
    seed, ocfg, batches = _three_batches()
    cfg, model = G.drn_model(ocfg, seed, "cuda", 5, "fp32")
    model.train()
    assert model.roi_heads.box_head.dropout_p > 0
    torch.manual_seed(5)
    eng = model.roi_heads._engine

    def fwd():
        out = {k: float(v.detach()) for k, v in model(batches[0]).items()}
        torch.cuda.synchronize()
        return out

    a = fwd()
    c1 = int(eng.seed_dev.item())
    b = fwd()
    c2 = int(eng.seed_dev.item())
    assert c1 != 0 and c2 == 2 * c1          # advanced once per forward, by the same increment
    assert a != b                            # fresh masks
    eng.seed_dev.zero_()
    assert fwd() == a                        # same counter, same masks
