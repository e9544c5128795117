"""CPU side of the per-step metrics ring (include/drn_wsod.h "per-step metrics"): the boundary (header, signature table,
exported symbols), MetricsRing's decoding on hand-built ring contents, the EventStorage additions and the writers, and the order
rule of enable_metrics()."""
import json
import os
import re
import subprocess
import types
import weakref

import numpy as np
import pytest
import torch

import golden_util as G
import metrics_util as MU
from __graft_entry__ import build, load_package

NAMES = ("drn_head_metrics", "drn_metrics_record")


@pytest.fixture(scope="module")
def pkg():
    return build()


def _mods():
    load_package()
    import importlib

    return (importlib.import_module("drn_wsod_pytorch_amd.metrics"), importlib.import_module("drn_wsod_pytorch_amd.events"),
            importlib.import_module("drn_wsod_pytorch_amd.ops"))


# ----------------------------------------------------------------------------------------------------------- the boundary
def test_header_signatures_and_exports_agree(pkg):
    hdr = open(os.path.join(G.ROOT, "include", "drn_wsod.h")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    nm = subprocess.run(["nm", "-D", "--defined-only", pkg._cabi.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = {ln.split()[-1] for ln in nm.splitlines()}
    kind = {"p": "*", "i": "int", "l": "long"}
    for name in NAMES:
        m = re.search(r"\bint\s+%s\s*\(([^;]*?)\)\s*;" % name, code, flags=re.S)
        assert m, "include/drn_wsod.h does not declare %s" % name
        args = [a.strip() for a in m.group(1).split(",")]
        sig = pkg._cabi._SIGS[name]
        assert len(args) == len(sig), (name, args, sig)
        for a, c in zip(args, sig):  # pointer / int / long, argument for argument
            if c == "p":
                assert "*" in a, (name, a)
            else:
                assert "*" not in a and re.match(r"(unsigned\s+)?%s\b" % kind[c], a), (name, a, c)
        assert name in exported and name in pkg._cabi.exported_symbols()
        assert hasattr(pkg._cabi.lib(), name)
    _, _, ops = _mods()
    for macro, val in (("MAX_HEADS", ops.METRICS_MAX_HEADS), ("MAX_LOSSES", ops.METRICS_MAX_LOSSES),
                       ("COUNTERS", ops.METRICS_COUNTERS), ("COUNT_STRIDE", ops.METRICS_COUNT_STRIDE),
                       ("ROWS_PER_BLOCK", ops.METRICS_ROWS_PER_BLOCK), ("RECORD_WORDS", ops.METRICS_RECORD_WORDS)):
        assert re.search(r"#define DRN_METRICS_%s %d\b" % (macro, val), hdr), macro
    assert [ops.head_metrics_rows(K) for K in (1, 5, 20, 80, 1023)] == [(32, 64), (16, 64), (8, 64), (2, 64), (1, 64)]


# ------------------------------------------------------------------------------------------------------------- decoding
W = 72


def _record(idx, losses, counts=(), M=0, last=None):
    """one record as the header lays it out, built by hand"""
    r = [0] * W
    r[0], r[1], r[2], r[3] = idx, len(losses), len(counts), M
    for i, v in enumerate(losses):
        r[4 + i] = MU.f32_bits(v)
    for k, row in enumerate(counts):
        r[20 + 6 * k: 26 + 6 * k] = list(row)
    r[W - 1] = idx if last is None else last
    return r


def _host(S, count, records):
    """host copy [4 + S * W]: state[0] = count, record i in slot i % S"""
    words = [0] * (4 + S * W)
    words[0] = count
    for r in records:
        s = r[0] % S
        words[4 + s * W: 4 + (s + 1) * W] = r
    return torch.from_numpy(np.array(words, dtype=np.uint32).view(np.int32).copy())


def _ring(S, names, n_img=1, iter0=0):
    M, _, _ = _mods()
    ring = M.MetricsRing(S, "cpu")
    ring.names, ring.n_img, ring.iter0 = list(names), n_img, iter0
    return ring


def test_wrap_around_reports_what_was_lost():
    """S = 4, count = 6: records 2..5 come out, records 0 and 1 are reported lost; a second decode of the same copy adds nothing"""
    ring = _ring(4, ["loss_cls"], iter0=100)
    host = _host(4, 6, [_record(i, [0.5 + i]) for i in range(6)])
    recs, lost = ring.decode(host)
    assert lost == 2
    assert [it for it, _ in recs] == [102, 103, 104, 105]  # iter0 + record index
    assert [r["loss_cls"] for _, r in recs] == [2.5, 3.5, 4.5, 5.5]
    assert [r["total_loss"] for _, r in recs] == [2.5, 3.5, 4.5, 5.5]
    assert ring.decode(host) == ([], 0)
    # three more steps: only the new records
    host = _host(4, 9, [_record(i, [0.5 + i]) for i in range(9)])
    recs, lost = ring.decode(host)
    assert lost == 0 and [it for it, _ in recs] == [106, 107, 108]


def test_a_slot_whose_index_words_disagree_is_rejected():
    ring = _ring(4, ["a"])
    recs = [_record(0, [1.0]), _record(1, [2.0], last=0), _record(2, [3.0])]
    out, lost = ring.decode(_host(4, 3, recs))
    assert [it for it, _ in out] == [0, 2] and lost == 1
    # a slot still holding an OLDER record (both words agree with each other, not with the expected index) is rejected too
    ring = _ring(4, ["a"])
    stale = _record(1, [2.0])
    host = _host(4, 6, [_record(i, [1.0]) for i in (2, 3, 4)] + [stale])  # slot 1 should hold record 5
    out, lost = ring.decode(host)
    assert [it for it, _ in out] == [2, 3, 4] and lost == 2 + 1


def test_ratios_and_omission_rules():
    """n / n_img; cls_accuracy only if M > 0; fg_cls_accuracy and false_negative only if n_fg > 0; total_loss = the Python-float sum
    in list order; bit patterns survive (NaN, inf)"""
    names = ["loss_cls", "loss_cls_r0", "loss_cls_r1"]
    ring = _ring(8, names, n_img=2, iter0=7)
    losses = [0.1, 1e-8, 3.25]
    counts = [(3, 30, 15, 20, 9, 4), (8, 40, 0, 40, 0, 0)]  # n_ig, n_bg, n_fg, n_acc, n_fg_acc, n_fneg; branch 1 has no foreground
    recs = [_record(0, losses, counts, M=48), _record(1, [float("nan"), float("inf"), 1.0], [(0, 0, 0, 0, 0, 0)] * 2, M=0)]
    out, lost = ring.decode(_host(8, 2, recs))
    assert lost == 0 and [it for it, _ in out] == [7, 8]
    r = out[0][1]
    f = [float(np.float32(v)) for v in losses]
    assert [r[n] for n in names] == f and r["total_loss"] == (0.0 + f[0]) + f[1] + f[2]
    assert r["roi_head/num_fg_samples_r0"] == 15 / 2 and r["roi_head/num_bg_samples_r0"] == 30 / 2
    assert r["roi_head/num_ig_samples_r0"] == 3 / 2 and r["roi_head/num_ig_samples_r1"] == 4.0
    assert r["fast_rcnn/cls_accuracy_r0"] == 20 / 48 and r["fast_rcnn/cls_accuracy_r1"] == 40 / 48
    assert r["fast_rcnn/fg_cls_accuracy_r0"] == 9 / 15 and r["fast_rcnn/false_negative_r0"] == 4 / 15
    assert "fast_rcnn/fg_cls_accuracy_r1" not in r and "fast_rcnn/false_negative_r1" not in r
    assert r == dict(MU.scalars(counts, 48, 2), total_loss=r["total_loss"], **dict(zip(names, f)))
    r = out[1][1]
    assert np.isnan(r["loss_cls"]) and r["loss_cls_r0"] == float("inf") and np.isnan(r["total_loss"])
    assert not any(k.startswith("fast_rcnn/") for k in r)  # M == 0: no accuracy at all
    assert r["roi_head/num_fg_samples_r0"] == 0.0


def test_a_record_with_another_loss_count_is_an_error():
    from drn_wsod_pytorch_amd._cabi import DrnError

    ring = _ring(4, ["a", "b"])
    with pytest.raises(DrnError):
        ring.decode(_host(4, 1, [_record(0, [1.0])]))


def test_collect_without_a_drain_is_empty():
    assert _ring(4, ["a"]).collect() == ([], 0)


# ---------------------------------------------------------------------------------------------------- storage and writers
def test_put_scalar_at_keeps_latest_and_history_consistent():
    _, E, _ = _mods()
    st = E.EventStorage(start_iter=10)
    st.put_scalar("a", 1.0)           # iteration 10, the existing way
    st.put_scalar_at("a", 3.0, 12)
    st.put_scalar_at("a", 2.0, 11)    # arrives late: the history stays ordered, latest stays the value of iteration 12
    st.put_scalar_at("b", 5.0, 3)
    assert st.history("a") == [(1.0, 10), (2.0, 11), (3.0, 12)]
    assert st.latest() == {"a": 3.0, "b": 5.0}
    st.put_scalar_at("a", 4.0, 12)    # the same iteration again: behind the earlier one
    assert st.history("a")[-1] == (4.0, 12) and st.latest()["a"] == 4.0
    assert st.latest_iter() == 12 and st.iter == 10


def test_median_window():
    """latest_with_smoothing_hint: np.median of the last window_size values (detectron2/utils/events.py:359-370, HistoryBuffer.median)"""
    _, E, _ = _mods()
    st = E.EventStorage()
    vals = [5.0, 1.0, 9.0, 3.0, 7.0, 2.0, 8.0]
    for i, v in enumerate(vals):
        st.put_scalar_at("x", v, i)
        st.put_scalar_at("lr", 0.1 * i, i, smoothing_hint=False)
    for w in (1, 2, 3, 4, 20):
        got = st.latest_with_smoothing_hint(w)
        assert got["x"] == float(np.median(vals[-w:])), w
        assert got["lr"] == 0.1 * 6
    st.put_scalar("y", torch.tensor(2.5))  # the existing put_scalar: smoothed by default, tensors floated on demand
    assert st.latest_with_smoothing_hint(3)["y"] == 2.5


def test_json_writer_lines_byte_for_byte(tmp_path):
    """the reference's line: json.dumps({"iteration": it, **scalars}, sort_keys=True) + "\\n" with the smoothed scalars"""
    _, E, _ = _mods()
    st = E.EventStorage()
    path = str(tmp_path / "metrics.json")
    w = E.JSONWriter(path, window_size=3)
    script = [(0, 4.0, 0.5), (1, 2.0, 0.25), (2, 9.0, 0.125), (3, 1.0, 0.0625)]
    want = []
    for it, tot, acc in script:
        st.put_scalar_at("total_loss", tot, it)
        st.put_scalar_at("fast_rcnn/cls_accuracy_r0", acc, it)
        st.put_scalar_at("lr", 0.01, it, smoothing_hint=False)
        E.write_all([w], st, it)
    w.close()
    want = ['{"fast_rcnn/cls_accuracy_r0": 0.5, "iteration": 0, "lr": 0.01, "total_loss": 4.0}\n',
            '{"fast_rcnn/cls_accuracy_r0": 0.375, "iteration": 1, "lr": 0.01, "total_loss": 3.0}\n',
            '{"fast_rcnn/cls_accuracy_r0": 0.25, "iteration": 2, "lr": 0.01, "total_loss": 4.0}\n',
            '{"fast_rcnn/cls_accuracy_r0": 0.125, "iteration": 3, "lr": 0.01, "total_loss": 2.0}\n']
    assert open(path).read() == "".join(want)
    assert [json.loads(l)["iteration"] for l in want] == [0, 1, 2, 3]
    # without an explicit iteration the storage's current one is written, inside a `with storage` block like the reference
    st.iter = 41
    w = E.JSONWriter(path, window_size=1)
    with st:
        w.write()
    w.close()
    assert json.loads(open(path).read().splitlines()[-1]) == {"iteration": 41, "fast_rcnn/cls_accuracy_r0": 0.0625, "lr": 0.01,
                                                               "total_loss": 1.0}


def test_common_metric_printer_line():
    _, E, _ = _mods()
    st = E.EventStorage()
    for it in range(25):
        st.put_scalar_at("total_loss", float(it), it)
        st.put_scalar_at("loss_cls_r0", 0.5, it)
        st.put_scalar_at("fast_rcnn/cls_accuracy_r0", 0.9, it)
        st.put_scalar_at("lr", 0.001 * (it + 1), it, smoothing_hint=False)
    lines = []
    p = E.CommonMetricPrinter(100, sink=lines.append)
    p.write(st, 24)
    # medians over the last 20 values (5 .. 24 -> 14.5), lr as put last, only names with "loss" in them
    assert lines == [" iter: 24  total_loss: 14.500  loss_cls_r0: 0.500  lr: 0.025000"]
    st2 = E.EventStorage(start_iter=3)
    st2.put_scalar_at("total_loss", 1.0, 3)
    assert p.format(st2) == " iter: 3  total_loss: 1.000  lr: N/A"


# --------------------------------------------------------------------------------------------------------------- order rule
def test_enable_metrics_after_priming_is_refused():
    """on a stub engine: a live `captured_by` (set by a graphed step when it is primed) makes enable_metrics() raise and name the
    order; without one, or once the step object is gone, a ring is attached"""
    load_package()
    from drn_wsod_pytorch_amd._cabi import DrnError
    from drn_wsod_pytorch_amd.modeling.roi_heads import OICRROIHeads

    class Step:
        pass

    step = Step()
    eng = types.SimpleNamespace(captured_by=weakref.ref(step), arena_w=torch.zeros(1), ensure=lambda dev: None, metrics=None)
    heads = types.SimpleNamespace(_engine=eng, parameters=lambda: iter([torch.zeros(1)]))
    with pytest.raises(DrnError, match=r"enable_metrics\(\), then create and prime"):
        OICRROIHeads.enable_metrics(heads)
    assert eng.metrics is None
    del step
    ring = OICRROIHeads.enable_metrics(heads, slots=5)
    assert eng.metrics is ring and ring.slots == 5 and ring.host.numel() == 4 + 5 * W
    OICRROIHeads.disable_metrics(heads)
    assert eng.metrics is None
