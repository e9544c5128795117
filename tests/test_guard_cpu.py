"""The anomaly guard (FusedSGD(nonfinite=...): skip the update on a non-finite loss), the parts that need no GPU: the C ABI of the
five entry points, mode validation, the multi-rank refusals, and Trainer.check_finite() exactly as it was with the guard off."""
import ctypes
import os
import re

import pytest
import torch

import golden_util as G
from __graft_entry__ import build, load_package

load_package()
from drn_wsod_pytorch_amd._cabi import DrnError  # noqa: E402
from drn_wsod_pytorch_amd.engine import FusedSGD, Trainer, build_optimizer  # noqa: E402
from drn_wsod_pytorch_amd.modeling import build_model  # noqa: E402

GUARDED = {"drn_sgd_step_guard": "drn_sgd_step_clip", "drn_sgd_step_block_guard": "drn_sgd_step_block_clip",
           "drn_gemm_tn_sgd_guard": "drn_gemm_tn_sgd", "drn_gemm_tn_acc_sgd_guard": "drn_gemm_tn_acc_sgd"}


def _cpu_model():
    cfg = G.drn_cfg(G.MODEL_CASES["model_r50c4_tiny"], "cpu")
    return cfg, build_model(cfg)


def _decl(hdr, name):
    m = re.search(r"\bint\s+%s\s*\(([^;]*)\);" % name, hdr)
    assert m, "include/drn_wsod.h does not declare %s" % name
    return [a.strip() for a in m.group(1).replace("\n", " ").split(",")]


def test_guard_entry_points_declared_and_exported():
    pkg = build()
    hdr = open(os.path.join(G.ROOT, "include", "drn_wsod.h")).read()
    lib = ctypes.CDLL(pkg._cabi.LIB_PATH)
    for name, plain in GUARDED.items():
        args, base = _decl(hdr, name), _decl(hdr, plain)
        # the unguarded entry point with ONE more argument, in front of the stream
        assert args[:-2] == base[:-1] and args[-2] == "const int* guard" and args[-1] == base[-1] == "void* stream", name
        assert hasattr(lib, name) and name in pkg._cabi.exported_symbols()
        assert len(pkg._cabi._SIGS[name]) == len(args)
        assert pkg._cabi._SIGS[name] == pkg._cabi._SIGS[plain][:-1] + "pp"
    args = _decl(hdr, "drn_loss_guard")
    assert args == ["const void* const* losses", "int n", "int mode", "int window_first", "int* state", "void* stream"]
    assert hasattr(lib, "drn_loss_guard") and len(pkg._cabi._SIGS["drn_loss_guard"]) == len(args)
    # the plain entry points keep their signatures (supersets are added, nothing is changed)
    assert len(_decl(hdr, "drn_sgd_step_clip")) == 16 and len(_decl(hdr, "drn_gemm_tn_sgd")) == 19


def test_nonfinite_mode_validation():
    cfg, model = _cpu_model()
    with pytest.raises(ValueError, match="nonfinite"):
        FusedSGD(model, 0.01, 0.9, 5e-4, nonfinite="ignore")
    with pytest.raises(ValueError, match="nonfinite"):
        build_optimizer(cfg, model, nonfinite=True)
    off = build_optimizer(cfg, model)
    assert off.nonfinite == "off" and off.guard_state() is None and off._gs is None
    assert model.roi_heads._engine.loss_guard is None
    assert off.raise_if_nonfinite() is None
    assert not hasattr(cfg.SOLVER, "NONFINITE") and not hasattr(cfg.WSL, "NONFINITE")  # an argument, never a config key
    for mode in ("raise", "skip"):
        opt = build_optimizer(cfg, model, nonfinite=mode)
        assert opt.nonfinite == mode and model.roi_heads._engine.loss_guard is opt._guard
        st = opt.guard_state()
        assert st == {"mode": mode, "skip": False, "calls": 0, "first_bad": -1, "bad": 0, "first_bad_iteration": None}
        assert opt._gs.dtype == torch.int32 and opt._gs.tolist() == [0, 0, -1, 0]
        opt.state_dict()  # nothing bad so far: saves
    # what "raise" does with a bad state: the reference's message, the FIRST bad iteration, and no checkpoint
    opt = build_optimizer(cfg, model, nonfinite="raise")
    tr = Trainer(cfg, model, iter([]), optimizer=opt, start_iter=100)
    opt._guard.state.copy_(torch.tensor([1, 7, 2, 5], dtype=torch.int32))
    with pytest.raises(FloatingPointError, match=r"^Loss became infinite or NaN at iteration=102!$"):
        tr.check_finite()
    with pytest.raises(FloatingPointError, match="iteration=102"):
        opt.state_dict()
    # "skip" never raises and reports the counts
    opt = build_optimizer(cfg, model, nonfinite="skip")
    tr = Trainer(cfg, model, iter([]), optimizer=opt, start_iter=100)
    opt._guard.state.copy_(torch.tensor([0, 7, 2, 5], dtype=torch.int32))
    st = tr.check_finite()
    assert (st["calls"], st["first_bad"], st["bad"], st["first_bad_iteration"], st["skip"]) == (7, 2, 5, 102, False)
    opt.state_dict()


def test_guard_refuses_more_than_one_rank():
    cfg, model = _cpu_model()

    class DP:
        world, exchange, group = 2, True, None
        grad_scale, sync_gradients = 0.5, True

    for mode in ("raise", "skip"):
        opt = build_optimizer(cfg, model, nonfinite=mode)
        with pytest.raises(DrnError, match="nonfinite.*gradient exchange"):
            opt.enable_pipelined(DP())
        with pytest.raises(DrnError, match="nonfinite.*K-sharded"):
            opt.enable_pipelined(None, exchange="fc6_kshard")
        with pytest.raises(DrnError, match="nonfinite.*gradient exchange"):
            Trainer(cfg, model, iter([]), optimizer=opt, parallel=DP())
        opt.enable_pipelined()  # single process: built
        Trainer(cfg, model, iter([]), optimizer=opt)
    # guard off: the same calls are today's
    opt = build_optimizer(cfg, model)
    Trainer(cfg, model, iter([]), optimizer=opt, parallel=DP())


def test_check_finite_unchanged_with_the_guard_off():
    cfg, model = _cpu_model()
    tr = Trainer(cfg, model, iter([]), optimizer=build_optimizer(cfg, model), start_iter=40)
    assert tr.check_finite() is None  # nothing ran yet
    tr.last_losses = {"loss_cls": torch.tensor(1.5), "loss_cls_r0": torch.tensor(0.25)}
    assert tr.check_finite() is None
    tr.iter = 43
    for bad in (float("nan"), float("inf")):
        tr.last_losses = {"loss_cls": torch.tensor(1.5), "loss_cls_r0": torch.tensor(bad)}
        with pytest.raises(FloatingPointError, match=r"^Loss became infinite or NaN at iteration=43!$"):
            tr.check_finite()
    tr.last_losses = {"a": torch.tensor(float("inf")), "b": torch.tensor(float("-inf"))}  # the SUM is tested
    with pytest.raises(FloatingPointError):
        tr.check_finite()
