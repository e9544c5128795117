"""Gradient accumulation (WSL.ITER_SIZE > 1) on the pipelined optimizer, the parts that need no GPU: the C ABI of the closing
launch (drn_gemm_tn_acc_sgd), FusedSGD.enable_pipelined(iter_size=N), the Trainer's guard, and the window positions the Trainer
hands to the optimizer (projects/WSL/tools/train_net.py:100-113: the optimizer steps when iter % N == 0)."""
import ctypes
import os
import re

import pytest
import torch

import golden_util as G
from __graft_entry__ import build, load_package

load_package()
from drn_wsod_pytorch_amd._cabi import DrnError  # noqa: E402
from drn_wsod_pytorch_amd.engine import Trainer, Window, build_optimizer, window_position  # noqa: E402
from drn_wsod_pytorch_amd.modeling import build_model  # noqa: E402


def _cpu_model():
    cfg = G.drn_cfg(G.MODEL_CASES["model_r50c4_tiny"], "cpu")
    return cfg, build_model(cfg)


def test_acc_sgd_entry_declared_and_exported():
    pkg = build()
    hdr = open(os.path.join(G.ROOT, "include", "drn_wsod.h")).read()
    m = re.search(r"\bint\s+drn_gemm_tn_acc_sgd\s*\(([^;]*)\);", hdr)
    assert m, "include/drn_wsod.h does not declare drn_gemm_tn_acc_sgd"
    args = [a.strip() for a in m.group(1).replace("\n", " ").split(",")]
    assert "const float* grad_acc" in args and "long ld_acc" in args
    # drn_gemm_tn_sgd with one more operand and its pitch
    m0 = re.search(r"\bint\s+drn_gemm_tn_sgd\s*\(([^;]*)\);", hdr)
    assert len(args) == len(m0.group(1).split(",")) + 2
    lib = ctypes.CDLL(pkg._cabi.LIB_PATH)
    assert hasattr(lib, "drn_gemm_tn_acc_sgd")
    assert "drn_gemm_tn_acc_sgd" in pkg._cabi.exported_symbols()
    assert len(pkg._cabi._SIGS["drn_gemm_tn_acc_sgd"]) == len(args)
    import importlib

    assert hasattr(importlib.import_module("drn_wsod_pytorch_amd.ops"), "gemm_tn_acc_sgd")


def test_enable_pipelined_iter_size_and_trainer_guard():
    cfg, model = _cpu_model()
    opt = build_optimizer(cfg, model)
    assert opt.iter_size == 1
    opt.enable_pipelined(iter_size=4)
    assert opt.iter_size == 4
    with pytest.raises(AttributeError):
        opt.iter_size = 2  # read-only
    eng = model.roi_heads._engine
    assert eng.accum_small and eng.accum_window is None and not eng.defer_colsum
    cfg.WSL.ITER_SIZE = 4
    tr = Trainer(cfg, model, iter([]), optimizer=opt)
    assert tr.iter_size == 4
    cfg.WSL.ITER_SIZE = 2
    with pytest.raises(DrnError, match="ITER_SIZE"):
        Trainer(cfg, model, iter([]), optimizer=opt)
    # back to no accumulation: today's state of the engine
    opt.enable_pipelined()
    assert opt.iter_size == 1 and not eng.accum_small and eng.defer_colsum
    with pytest.raises(DrnError):
        opt.set_window(Window(True, True))
    with pytest.raises(DrnError):
        opt.enable_pipelined(iter_size=0)


def test_iter_size_refuses_what_is_not_built():
    cfg, model = _cpu_model()
    opt = build_optimizer(cfg, model)

    class DP:
        world, exchange, group = 1, True, None

    with pytest.raises(DrnError, match="ITER_SIZE"):
        opt.enable_pipelined(DP(), iter_size=4)
    with pytest.raises(DrnError, match="ITER_SIZE"):
        opt.enable_pipelined(None, exchange="fc6_kshard", iter_size=4)
    cfg3 = G.drn_cfg(G.MODEL_CASES["model_r50c4_tiny"], "cpu", freeze_at=3)
    opt3 = build_optimizer(cfg3, build_model(cfg3))
    with pytest.raises(DrnError, match="ITER_SIZE"):
        opt3.enable_pipelined(iter_size=4)


def test_window_position_rule():
    N = 4
    # start_iter = 0: windows {0}, {1..4}, {5..8}
    pos = [window_position(i, N, 0) for i in range(9)]
    assert [p.closing for p in pos] == [i % N == 0 for i in range(9)]
    assert [p.first for p in pos] == [True, True, False, False, False, True, False, False, False]
    # resumed at 7: the run starts from cleared gradients, the first optimizer step is behind iteration 8
    pos = [window_position(i, N, 7) for i in range(7, 14)]
    assert [p.closing for p in pos] == [i % N == 0 for i in range(7, 14)]
    assert [p.first for p in pos] == [True, False, True, False, False, False, True]
    # every window has exactly one first and one closing micro-iteration, first before closing
    for start in (0, 7):
        seen_first = False
        for i in range(start, start + 40):
            p = window_position(i, N, start)
            if p.first:
                assert not seen_first
                seen_first = True
            assert seen_first
            if p.closing:
                seen_first = False


class _StubPipelinedOpt:
    """what Trainer.run_step needs of a pipelined FusedSGD"""
    _pipelined = True

    def __init__(self, iter_size):
        self.iter_size = iter_size
        self.param_groups = [{"lr": 0.01, "initial_lr": 0.01}]
        self.log = []

    def set_window(self, win):
        self.log.append(("win", win))

    def step(self, scale=1.0):
        self.log.append("step")

    def zero_grad(self):
        pass


@pytest.mark.parametrize("start", [0, 7])
def test_trainer_hands_the_window_position_to_the_optimizer(start):
    cfg, _ = _cpu_model()
    cfg.WSL.ITER_SIZE = 4
    w = torch.zeros((), requires_grad=True)
    events = []

    class M:
        training = True

        def __call__(self, data):
            return {"loss_cls": (w * 2.0).sum()}

        def backward_losses(self, scale):
            events.append(("backward", scale))
            return True

    class Inst:
        def __len__(self):
            return 1

    def it():
        while True:
            yield [{"instances": Inst()}]

    class DP:
        grad_scale, sync_gradients = 1.0, True

        def finish(self):
            pass

    opt = _StubPipelinedOpt(4)
    opt.log = events
    tr = Trainer(cfg, M(), it(), optimizer=opt, parallel=DP(), start_iter=start)
    n = 10
    for _ in range(n):
        tr.run_step()
    i = start
    k = 0
    while i < start + n:
        # the position is set BEFORE the backward, the backward carries 1 / N, the step follows on closing iterations only
        assert events[k] == ("win", window_position(i, 4, start)), (i, events[k])
        assert events[k + 1] == ("backward", 0.25)
        k += 2
        if i % 4 == 0:
            assert events[k] == "step", i
            k += 1
        i += 1
    assert k == len(events)
    with pytest.raises(DrnError, match="ITER_SIZE"):
        Trainer(cfg, M(), it(), optimizer=_StubPipelinedOpt(2), parallel=DP())
