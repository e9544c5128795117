"""The padded inference tail and the dataset loop, the parts that need no GPU: DetectionBatch on CPU tensors,
inference_on_dataset / DatasetEvaluators / inference_context with a fake model and a recording evaluator, the alias module,
and the C ABI of the three new entries (header, exports, _cabi)."""
import ctypes
import fnmatch
import importlib
import os
import re
import subprocess

import pytest
import torch

import golden_util as G
from __graft_entry__ import build, load_package

load_package()
from drn_wsod_pytorch_amd import evaluation as E  # noqa: E402
from drn_wsod_pytorch_amd import ops  # noqa: E402
from drn_wsod_pytorch_amd._cabi import DrnError  # noqa: E402
from drn_wsod_pytorch_amd.structures import DetectionBatch, Instances  # noqa: E402


def test_detection_batch_to_instances_on_cpu_tensors():
    N, topk = 3, 5
    boxes = torch.arange(N * topk * 4, dtype=torch.float32).reshape(N, topk, 4)
    scores = torch.arange(N * topk, dtype=torch.float32).reshape(N, topk) / 10
    classes = (torch.arange(N * topk, dtype=torch.int32).reshape(N, topk) % 4)
    count = torch.tensor([2, 0, 5], dtype=torch.int32)
    batch = DetectionBatch(boxes, scores, classes, count, [(10, 20), (30, 40), [50, 60]])
    assert len(batch) == 3 and batch.topk == topk and batch.image_sizes == [(10, 20), (30, 40), (50, 60)]
    inst = batch.to_instances()
    assert [len(r) for r in inst] == [2, 0, 5] and all(isinstance(r, Instances) for r in inst)
    for i, r in enumerate(inst):
        n = int(count[i])
        assert r.image_size == batch.image_sizes[i]
        assert torch.equal(r.pred_boxes.tensor, boxes[i, :n]) and torch.equal(r.scores, scores[i, :n])
        assert r.pred_classes.dtype == torch.int64 and torch.equal(r.pred_classes, classes[i, :n].long())
    outs = batch.to_outputs()
    assert [sorted(o) for o in outs] == [["instances"]] * 3 and len(outs[2]["instances"]) == 5
    with pytest.raises(AssertionError):
        DetectionBatch(boxes, scores, classes, count, [(10, 20)])  # one size per image


class Recorder:
    def __init__(self, log, name="ev", result="default"):
        self.log, self.name = log, name
        self.result = {name: {"AP": 1.0}} if result == "default" else result

    def reset(self):
        self.log.append((self.name, "reset"))

    def process(self, inputs, outputs):
        self.log.append((self.name, "process", inputs, outputs))

    def evaluate(self):
        self.log.append((self.name, "evaluate"))
        return self.result


class FakeModel(torch.nn.Module):
    def __init__(self, log, fail_at=None):
        super().__init__()
        self.sub = torch.nn.Linear(1, 1)
        self.log, self.fail_at, self.calls = log, fail_at, 0

    def forward(self, inputs):
        assert not self.training and not self.sub.training and not torch.is_grad_enabled()
        if self.calls == self.fail_at:
            raise RuntimeError("boom")
        self.calls += 1
        self.log.append(("model", inputs))
        return ("out", inputs)


def test_inference_on_dataset_call_order_and_mode():
    log = []
    model = FakeModel(log)
    model.train()
    res = E.inference_on_dataset(model, ["a", "b", "c"], Recorder(log))
    assert res == {"ev": {"AP": 1.0}}
    assert log == [("ev", "reset"), ("model", "a"), ("ev", "process", "a", ("out", "a")), ("model", "b"),
                   ("ev", "process", "b", ("out", "b")), ("model", "c"), ("ev", "process", "c", ("out", "c")), ("ev", "evaluate")]
    assert model.training and model.sub.training  # restored
    model.eval()
    E.inference_on_dataset(model, ["a"], Recorder(log))
    assert not model.training  # an eval model stays in eval mode


def test_inference_on_dataset_none_results_and_no_evaluator():
    log = []
    assert E.inference_on_dataset(FakeModel(log), ["a"], Recorder(log, result=None)) == {}
    model = FakeModel(log)
    assert E.inference_on_dataset(model, ["a", "b"], None) == {} and model.calls == 2


def test_mode_is_restored_when_the_model_raises():
    log = []
    model = FakeModel(log, fail_at=1)
    model.train()
    with pytest.raises(RuntimeError):
        E.inference_on_dataset(model, ["a", "b"], Recorder(log))
    assert model.training and model.sub.training
    assert ("ev", "evaluate") not in log
    with pytest.raises(KeyError):
        with E.inference_context(model):
            assert not model.training
            raise KeyError("x")
    assert model.training


def test_dataset_evaluators_dispatch_and_merge():
    log = []
    both = E.DatasetEvaluators([Recorder(log, "a"), Recorder(log, "b"), Recorder(log, "c", result=None)])
    both.reset()
    both.process("in", "out")
    assert both.evaluate() == {"a": {"AP": 1.0}, "b": {"AP": 1.0}}
    assert [e[:2] for e in log] == [("a", "reset"), ("b", "reset"), ("c", "reset"), ("a", "process"), ("b", "process"),
                                    ("c", "process"), ("a", "evaluate"), ("b", "evaluate"), ("c", "evaluate")]
    with pytest.raises(AssertionError):
        E.DatasetEvaluators([Recorder(log, "a"), Recorder(log, "a")]).evaluate()
    assert E.DatasetEvaluators([]).evaluate() == {}


def test_alias_module_exposes_the_loop_and_still_refuses_coco():
    A = importlib.import_module("drn_wsod_pytorch_amd.aliases")
    A.install()
    try:
        mod = importlib.import_module("detectron2.evaluation")
        assert mod.inference_on_dataset is E.inference_on_dataset and mod.inference_context is E.inference_context
        assert mod.DatasetEvaluators is E.DatasetEvaluators
        assert mod.PascalVOCDetectionEvaluator is E.PascalVOCDetectionEvaluator
        with pytest.raises(DrnError) as err:
            mod.COCOEvaluator
        assert "COCOEvaluator" in str(err.value) and not hasattr(mod, "COCOEvaluator")
    finally:
        A.uninstall()
    import sys

    assert "detectron2" not in sys.modules


def test_limits_are_refused_without_a_device():
    """the host checks of detect_topk_batch come before anything touches the device"""
    n = ops.DETECT_MAX_IMAGES + 1
    with pytest.raises(DrnError):
        ops.detect_topk_batch(torch.zeros((n, 4)), torch.zeros((n, 4)), list(range(n + 1)), [(8, 8)] * n, None, score_thresh=0.1,
                              nms_thresh=0.3, topk=100)
    M = ops.DETECT_BATCH_MAX_ENTRIES // 4 + 1
    with pytest.raises(DrnError):
        ops.detect_topk_batch(torch.zeros((M, 4)), torch.zeros((M, 5)), [0, M], [(8, 8)], None, score_thresh=0.1,
                              nms_thresh=0.3, topk=100)
    with pytest.raises(DrnError):
        ops.detect_topk_batch(torch.zeros((4, 4)), torch.zeros((4, 5)), [0, 3], [(8, 8)], None, score_thresh=0.1, nms_thresh=0.3,
                              topk=100)  # img_off does not end at M


ENTRIES = {"drn_detect_topk_batch": 20, "drn_detect_compact": 14}


def _decl(hdr, name, ret="int"):
    m = re.search(r"\b%s\s+%s\s*\(([^;]*)\);" % (ret, name), hdr)
    assert m, "include/drn_wsod.h does not declare %s" % name
    return [" ".join(a.split()) for a in m.group(1).replace("\n", " ").split(",")]


def test_new_entries_declared_exported_and_bound():
    pkg = build()
    C = pkg._cabi
    hdr = open(os.path.join(G.ROOT, "include", "drn_wsod.h")).read()
    out = subprocess.check_output(["nm", "-D", "--defined-only", C.LIB_PATH], text=True)
    defined = {l.split()[-1] for l in out.splitlines() if l.strip()}
    emap = open(os.path.join(G.ROOT, "drn-wsod-pytorch_amd", "csrc", "exports.map")).read()
    globs = re.search(r"global:\s*([^;]*);", emap).group(1).split()
    lib = ctypes.CDLL(C.LIB_PATH)
    for name, nargs in ENTRIES.items():
        args = _decl(hdr, name)
        assert len(args) == nargs and args[-1] == "void* stream", (name, args)
        sig = C._SIGS[name]
        assert len(sig) == len(args)
        for ch, a in zip(sig, args):
            want = "p" if "*" in a else "f" if a.startswith("float") else "l" if a.startswith("long") else "i"
            assert ch == want, (name, a, ch)
    assert _decl(hdr, "drn_detect_batch_workspace_bytes", "long") == ["int total_cap", "int n_images"]
    for name in list(ENTRIES) + ["drn_detect_batch_workspace_bytes"]:
        assert name in defined and hasattr(lib, name) and name in C.exported_symbols()
        assert any(fnmatch.fnmatchcase(name, g) for g in globs), "exports.map does not list %s" % name
    assert hasattr(ops, "detect_topk_batch") and hasattr(ops, "detections_compact")
    assert int(re.search(r"#define\s+DRN_DETECT_MAX_IMAGES\s+(\d+)", hdr).group(1)) == ops.DETECT_MAX_IMAGES >= 16
    assert int(re.search(r"#define\s+DRN_DETECT_BATCH_MAX_ENTRIES\s+(\d+)", hdr).group(1)) == ops.DETECT_BATCH_MAX_ENTRIES
    big = C.lib().drn_detect_batch_workspace_bytes(42000, 16)
    assert big > C.lib().drn_detect_workspace_bytes(42000) and big > C.lib().drn_detect_batch_workspace_bytes(42000, 1)
    # the single-image entries keep their argument lists
    assert C._SIGS["drn_detect_topk"] == "ppiii" + "ffff" + "i" + "pl" + "i" + "ppp" and C._SIGS["drn_detect_gather"] == "plippippppp"
