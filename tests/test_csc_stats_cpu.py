"""The CSC weight statistics (CSCROIHeads.enable_csc_stats, metrics.CscStats, ops.csc_stats / drn_csc_stats), the parts that
need no GPU: the text of the reference's csc.txt blocks from the recorded fixture of its unmodified `Statistic`
(tests/golden/csc_stats.npz, gen_golden_csc_stats.py), the period / max_iter rule, the engine's declared slot, the opt-in's
absence on the other heads, no launch with the option off, the C ABI and the limits refused on the host."""
import ctypes
import os
import re
import types

import numpy as np
import pytest
import torch

import csc_stats_util as U
import golden_util as G
from __graft_entry__ import build, load_package

load_package()
from drn_wsod_pytorch_amd import metrics, ops  # noqa: E402
from drn_wsod_pytorch_amd._cabi import DrnError  # noqa: E402
from drn_wsod_pytorch_amd.modeling import build_model, head_engine  # noqa: E402


@pytest.fixture(scope="module")
def fixture():
    d = G.load("csc_stats")
    steps = [{k: d["step%d_%s" % (it, k)] for k in ("scores", "W", "img_off", "onehot")} for it in range(int(d["steps"]))]
    return d, steps


def _fake_launch(tau):
    """ops.csc_stats without a device: the numpy restatement added to the table tensor's words"""
    def fake(scores, W, img_off, n_img, onehot, slots, table, scratch=None):
        K = scores.shape[1]
        t = metrics.decode_csc_stats(table.numpy(), K)
        for f in U.FP_FIELDS:
            t["bound_" + f] = np.zeros(K)
        sc, off, oh = scores.numpy(), img_off.numpy(), onehot.numpy().reshape(n_img, K)
        U.add_step(t, sc, W.numpy(), off, oh, U.active_of(sc, off, oh, tau))
        table.copy_(torch.from_numpy(U.to_words(t)))
        return table
    return fake


def test_format_reproduces_the_reference_blocks_byte_for_byte(fixture, monkeypatch, tmp_path):
    d, steps = fixture
    K, tau, period, max_iter = int(d["K"]), float(d["tau"]), int(d["period"]), int(d["max_iter"])
    want = [str(b) for b in d["blocks"]]
    iters = d["block_iters"].tolist()
    assert iters == [0, 4, 8] and len(steps) == 14 > max_iter + period  # forwards past max_iter are in the sequence
    # 1. the restatement's tables of each period, through format alone
    t, got = U.new_table(K), []
    for it, s in enumerate(steps):
        U.add_step(t, s["scores"], s["W"], s["img_off"], s["onehot"], U.active_of(s["scores"], s["img_off"], s["onehot"], tau))
        if it % period == 0 and it <= max_iter:
            got.append(metrics.CscStats.format(t, it))
            t = U.new_table(K)
    assert got == want, "\n".join(["GOT"] + got + ["WANT"] + want)
    # 2. the same through CscStats (table words, drain, re-zero, decode, the file), the launch replaced by the restatement
    monkeypatch.setattr(ops, "csc_stats", _fake_launch(tau))
    st = metrics.CscStats(K, max_iter, period, str(tmp_path), "x_", 0, "cpu")
    for s in steps:
        n_img = len(s["img_off"]) - 1
        st.forward(torch.from_numpy(s["scores"]), torch.from_numpy(s["W"]), torch.from_numpy(s["img_off"]), n_img,
                   torch.from_numpy(s["onehot"]), None)
    st.collect()
    assert [it for it, _ in st.blocks] == iters and [b for _, b in st.blocks] == want
    assert open(os.path.join(str(tmp_path), "x_csc.txt")).read() == "".join(b + "\n" for b in want)
    # the fixture covers what it says: a class never labelled, labelled below tau, only zero weights
    b0 = want[0].split("\n")
    assert b0[2].startswith("0\t0.0000\t0\t0\t0.0000") and b0[3].startswith("1\t0.46875\t7\t0\t0.0000")
    assert b0[4].endswith("\t7\t1.00000\t2") and "\t2.0\t" in b0[6]  # csc_acm_label printed as a float


def test_which_forwards_emit(monkeypatch):
    """LogIterStats: a block after the forward with cur_iter % period == 0 and cur_iter <= max_iter, counted from start_iter;
    a forward past CSC_MAX_ITER is counted but launches nothing"""
    calls = []
    monkeypatch.setattr(ops, "csc_stats", lambda *a, **k: calls.append(1))
    z = torch.zeros((3, 4))
    off = torch.tensor([0, 3], dtype=torch.int32)
    for period, max_iter, start, n, want in [(4, 9, 0, 14, [0, 4, 8]), (4, 8, 0, 14, [0, 4, 8]), (4, 7, 0, 14, [0, 4]),
                                             (3, 100, 5, 8, [6, 9, 12]), (1, 2, 0, 5, [0, 1, 2]), (320, 35000, 1, 700, [320, 640])]:
        st = metrics.CscStats(4, max_iter, period, None, "", start, "cpu")
        del calls[:]
        for i in range(n):
            st.forward(z, z, off, 1, z[:1], None, launch=start + i <= max_iter)
        assert st.cur_iter == start + n
        st.collect()
        assert [it for it, _ in st.blocks] == want, (period, max_iter, start, st.blocks)
        assert len(calls) == sum(1 for i in range(n) if start + i <= max_iter)
    # flush: the open period as a block labelled with the last forward, then nothing more
    st = metrics.CscStats(4, 100, 4, None, "", 0, "cpu")
    for i in range(6):
        st.forward(z, z, off, 1, z[:1], None)
    assert [it for it, _ in st.flush()] == [5] and st.flush() == []  # (0 and 4 were collected by the forwards behind them)
    assert [it for it, _ in st.blocks] == [0, 4, 5]
    with pytest.raises(DrnError):
        metrics.CscStats(4, 100, 0, None, "", 0, "cpu")


def test_slot_is_declared_and_the_option_is_a_method_of_csc_heads_only():
    assert "csc_stats" in head_engine._HeadEngine.__slots__
    cfg = G.drn_cfg(G.csc_case(), "cpu")
    heads = build_model(cfg).roi_heads
    assert type(heads).__name__ == "CSCROIHeads" and heads._engine.csc_stats is None
    assert head_engine._HeadEngine(heads).csc_stats is None
    assert not any("STAT" in k.upper() for k in cfg.WSL)  # a method, not a config key
    st = heads.enable_csc_stats(period=7, start_iter=3)
    assert isinstance(st, metrics.CscStats) and heads._engine.csc_stats is st
    assert (st.period, st.cur_iter, st.max_iter, st.K, st.path) == (7, 3, heads.csc_max_iter, heads.num_classes, None)
    assert heads.enable_csc_stats().period == 320  # LOG_PERIOD = 1280 / 4
    assert heads.enable_csc_stats(output_dir="out", prefix="r0_").path == os.path.join("out", "r0_csc.txt")
    heads.disable_csc_stats()
    assert heads._engine.csc_stats is None
    doc = type(heads).__doc__
    assert "log writer" not in doc and "enable_csc_stats" in doc
    for name in ("model_r50c4_tiny", "model_pcl_r50c4_tiny", "model_wsddn_r50c4_tiny"):
        other = build_model(G.drn_cfg(G.MODEL_CASES[name], "cpu")).roi_heads
        assert type(other).__name__ in ("OICRROIHeads", "PCLROIHeads", "WSDDNROIHeads")
        assert not hasattr(other, "enable_csc_stats") and not hasattr(other, "disable_csc_stats")
        assert other._engine.csc_stats is None


@pytest.mark.parametrize("batch", [False, True])
def test_no_launch_with_the_option_off(monkeypatch, batch):
    """_losses_csc / _losses_csc_batch with every launch replaced by a recorder: off = no csc_stats call and no upload; on = one
    call with the step's own active decision; past CSC_MAX_ITER = the forward is counted, nothing is launched"""
    heads = build_model(G.drn_cfg(G.csc_case(), "cpu")).roi_heads
    eng = heads._engine
    K, n = heads.num_classes, 2 if batch else 1
    heads.enable_image_batches(batch)
    rows = [3, 2][:n]
    M = sum(rows)
    calls = []
    scores = torch.full((M, K), 1.0 / 64)
    monkeypatch.setattr(ops, "wsddn_fwd_bwd", lambda *a, **k: (scores, torch.zeros((n, K)), None, scores))
    monkeypatch.setattr(ops, "csc_loss", lambda *a, **k: torch.zeros(2))
    monkeypatch.setattr(ops, "csc_loss_batch", lambda *a, **k: (torch.zeros((n, 2)), torch.zeros(2)))
    monkeypatch.setattr(ops, "csc_stats", lambda *a, **k: calls.append((a, k)))
    monkeypatch.setattr(head_engine._HeadEngine, "_finish", lambda self, s, names, col0s, **f: (names, f))
    plan = ops.CscBatchPlan([(8, 8)] * 2, K, [[1, 2], [-1, 3]], [(0, 1), (1, 2), (1, 3)], "cpu")

    def weights(*a, **k):
        if heads.iter > heads.csc_max_iter:
            heads._csc_sched = None
            return None, None
        heads._csc_sched = plan if batch else [1, 2]
        return torch.ones((M, K)), None

    monkeypatch.setattr(heads, "_csc_weights_batch" if batch else "_csc_weights", weights)
    s = types.SimpleNamespace(w={"logits": None, "dlogits": None}, col={"cls": 0, "det": K}, n_img=n, M=M, dtype=torch.float32,
                              gt={"onehot": torch.ones((n, K)), "max_rows": max(rows), "rows": rows}, fg=None, masks=None,
                              drop_p=0.0, img_off=torch.tensor([0] + list(np.cumsum(rows)), dtype=torch.int32))
    heads.iter, heads.csc_max_iter = 1, 5
    eng._losses_csc(s)
    assert calls == []  # off
    st = heads.enable_csc_stats(period=2)
    eng._losses_csc(s)
    assert len(calls) == 1 and st.cur_iter == 1
    a = calls[0][0]
    assert a[0] is scores and a[3] == n and a[6] is st.table
    assert a[5].tolist() == ([1, 2, -1, 3] if batch else [1, 2]) and a[5].dtype == torch.int64
    if batch:
        assert a[5].untyped_storage().data_ptr() == plan.words.untyped_storage().data_ptr()  # read from the plan's one upload
    heads.iter = 6  # past CSC_MAX_ITER: W is None
    eng._losses_csc(s)
    assert len(calls) == 1 and st.cur_iter == 2
    heads.disable_csc_stats()
    heads.iter = 1
    eng._losses_csc(s)
    assert len(calls) == 1


def test_entry_declared_exported_bound_and_limits_refused_on_the_host():
    pkg = build()
    C = pkg._cabi
    hdr = open(os.path.join(G.ROOT, "include", "drn_wsod.h")).read()
    m = re.search(r"\bint\s+drn_csc_stats\s*\(([^;]*)\);", hdr)
    args = [" ".join(a.split()) for a in m.group(1).replace("\n", " ").split(",")]
    sig = C._SIGS["drn_csc_stats"]
    assert len(args) == len(sig) == 12 and args[-1] == "void* stream"
    for ch, a in zip(sig, args):
        assert ch == ("p" if "*" in a else "i"), (a, ch)
    lib = ctypes.CDLL(C.LIB_PATH)
    assert hasattr(lib, "drn_csc_stats") and "drn_csc_stats" in C.exported_symbols()
    assert "CSC weight statistics" in hdr and "one `UpdateIterStats` call, in ascending image order" in hdr
    for name, val in (("HEAD", len(ops.CSC_STATS_HEAD)), ("INT", len(ops.CSC_STATS_INT)), ("FP", len(ops.CSC_STATS_FP))):
        assert int(re.search(r"#define\s+DRN_CSC_STATS_%s\s+(\d+)" % name, hdr).group(1)) == val
    assert ops.CSC_STATS_INT == U.INT_FIELDS and ops.CSC_STATS_FP == U.FP_FIELDS and ops.csc_stats_words(20) == 2 + 11 * 20
    z = torch.zeros
    with pytest.raises(DrnError, match="17 images"):
        ops.csc_stats(z(17, 20), z(17, 20), torch.arange(18, dtype=torch.int32), 17, z(17, 20), None,
                      z(ops.csc_stats_words(20), dtype=torch.int64))
    with pytest.raises(DrnError, match="K = 129"):
        ops.csc_stats(z(2, 129), z(2, 129), torch.arange(3, dtype=torch.int32), 2, z(2, 129), None,
                      z(ops.csc_stats_words(129), dtype=torch.int64))
    with pytest.raises(DrnError):  # no W: past CSC_MAX_ITER there is nothing to count
        ops.csc_stats(z(2, 20), None, torch.arange(3, dtype=torch.int32), 2, z(2, 20), None, z(ops.csc_stats_words(20), dtype=torch.int64))
    l = C.lib()
    assert l.drn_csc_stats(None, None, 20, None, 17, 17, None, None, 0, None, None, None) == -3
    assert l.drn_csc_stats(None, None, 129, None, 2, 2, None, None, 0, None, None, None) == -3
    assert l.drn_csc_stats(None, None, 20, None, 2, 2, None, None, 0, None, None, None) == -1
