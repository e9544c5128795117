"""CPU tests of the stand-alone box operators' host side: the alias names, the workspace formula, the refusals that must come before
the library is touched, the empty input, Matcher's constructor, and the generator's own promises (tests/nms_util.py)."""
import ctypes
import importlib
import re
import subprocess
import sys

import pytest
import torch

import golden_util as G
import nms_util as U
from __graft_entry__ import build


@pytest.fixture(scope="module")
def pkg():
    return build()


@pytest.fixture(scope="module")
def ops(pkg):
    return importlib.import_module("drn_wsod_pytorch_amd.ops")


def test_alias_names_resolve():
    code = """
import sys
sys.path.insert(0, %r)
from __graft_entry__ import load_package
load_package()
import drn_wsod_pytorch_amd.aliases as A
A.install()
from detectron2.layers import nms, batched_nms
from detectron2.structures import pairwise_iou, Boxes
from detectron2.modeling.matcher import Matcher
import drn_wsod_pytorch_amd.layers as L, drn_wsod_pytorch_amd.structures as S
assert nms is L.nms and batched_nms is L.batched_nms and pairwise_iou is S.pairwise_iou
assert callable(Matcher([0.5], [0, 1]))
try:
    from detectron2.utils import comm
except ImportError:
    pass
else:
    raise SystemExit("detectron2.utils.comm must stay off the path")
try:
    from detectron2.evaluation import COCOEvaluator
except ImportError:
    pass
else:
    raise SystemExit("detectron2.evaluation.COCOEvaluator must stay off the path")
print("ok")
""" % G.ROOT
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip() == "ok", r.stderr + r.stdout


def test_workspace_is_linear_in_n(ops, pkg):
    n0, n1, n2 = 2 ** 10, 2 ** 15, 2 ** 19
    b0, b1, b2 = (ops.nms_workspace_bytes(n) for n in (n0, n1, n2))
    assert (b1 - b0) * (n2 - n1) == (b2 - b1) * (n1 - n0)  # one slope: a * n + c
    slope = (b1 - b0) // (n1 - n0)
    assert slope * (n1 - n0) == b1 - b0 and 0 < slope <= 128 and 0 <= b0 - slope * n0 <= 1 << 20
    # the formula the header states
    hdr = open(G.ROOT + "/include/drn_wsod.h").read()
    m = re.search(r"#define DRN_NMS_WS_BYTES\(n\) \((\d+)L \* \(n\) \+ (\d+)L\)", hdr)
    assert m and all(int(m.group(1)) * n + int(m.group(2)) == b for n, b in ((n0, b0), (n1, b1), (n2, b2)))
    assert int(re.search(r"#define DRN_NMS_MAX_N (\d+)", hdr).group(1)) == ops.NMS_MAX_N >= 524288


class _Touched(Exception):
    pass


def _no_library(monkeypatch, pkg):
    def boom(*a, **k):
        raise _Touched("the library was touched")

    monkeypatch.setattr(pkg._cabi, "call", boom)
    monkeypatch.setattr(pkg._cabi, "lib", boom)


def test_refusals_come_before_the_library(ops, pkg, monkeypatch):
    _no_library(monkeypatch, pkg)
    E = pkg._cabi.DrnError
    big = ops.NMS_MAX_N + 1
    boxes, scores, idxs = torch.zeros(big, 4), torch.zeros(big), torch.zeros(big, dtype=torch.int64)
    for padded in (False, True):
        with pytest.raises(E, match="at most"):
            ops.nms(boxes, scores, 0.5, padded=padded)
        with pytest.raises(E, match="at most"):
            ops.batched_nms(boxes, scores, idxs, 0.5, padded=padded)
    with pytest.raises(E):
        ops.nms(torch.zeros(3, 5), torch.zeros(3), 0.5)
    with pytest.raises(E):
        ops.nms(torch.zeros(3, 4), torch.zeros(4), 0.5)
    with pytest.raises(E):
        ops.nms(torch.zeros(3, 4), torch.zeros(3), float("nan"))
    with pytest.raises(E):
        ops.batched_nms(torch.zeros(3, 4), torch.zeros(3), torch.zeros(2, dtype=torch.int64), 0.5)
    with pytest.raises(E, match="at most"):
        ops.detect_all(torch.zeros(26215, 4 * 20), torch.zeros(26215, 21), (10, 10), 0.05, 0.5)
    with pytest.raises(E):
        ops.detect_all(torch.zeros(3, 8), torch.zeros(3, 3), (10, 10), 0.05, 0.5, topk=0)
    with pytest.raises(E):
        ops.detect_all(torch.zeros(3, 12), torch.zeros(3, 3), (10, 10), 0.05, 0.5)
    with pytest.raises(E):
        ops.pairwise_iou(torch.zeros(3, 5), torch.zeros(3, 4))
    with pytest.raises(E):
        ops.match(torch.zeros(3, 4), [0.5], [0, 2])
    with pytest.raises(E):
        ops.match(torch.zeros(3, 4), [0.1, 0.2, 0.3, 0.4], [0, 0, 0, 0, 1])
    with pytest.raises(E):
        ops.match(torch.zeros(3, 4), [0.5], [0, 1, 1])
    # host tensors reach the binding only behind the checks (there is no CPU path: with a GPU they would be moved to it)
    with pytest.raises((_Touched, RuntimeError, AssertionError)):
        ops.nms(torch.zeros(3, 4), torch.zeros(3), 0.5)


def test_empty_input_needs_no_library(ops, pkg, monkeypatch):
    _no_library(monkeypatch, pkg)
    got = ops.nms(torch.zeros(0, 4), torch.zeros(0), 0.5)
    assert got.dtype == torch.int64 and got.shape == (0,)
    got = ops.batched_nms(torch.zeros(0, 4), torch.zeros(0), torch.zeros(0, dtype=torch.int64), 0.5)
    assert got.dtype == torch.int64 and got.shape == (0,)
    keep, count = ops.nms(torch.zeros(0, 4), torch.zeros(0), 0.5, padded=True)
    assert keep.dtype == torch.int64 and keep.shape == (0,) and count.dtype == torch.int32 and count.tolist() == [0]
    assert ops.pairwise_iou(torch.zeros(0, 4), torch.zeros(5, 4)).shape == (0, 5)
    assert ops.pairwise_iou(torch.zeros(5, 4), torch.zeros(0, 4)).shape == (5, 0)
    m, l = ops.match(torch.zeros(3, 0), [0.5], [0, 1])
    assert m.dtype == torch.int64 and l.dtype == torch.int8 and m.shape == l.shape == (0,)


def test_c_entries_refuse_before_any_launch(pkg):
    lib = pkg._cabi.lib()
    one = ctypes.c_int(5)
    p = ctypes.cast(ctypes.pointer(one), ctypes.c_void_p)
    assert lib.drn_nms(p, p, 524289, 0.5, p, 1 << 40, p, p, None) == -3       # beyond the cap
    assert lib.drn_batched_nms(p, p, p, 524289, 0.5, p, 1 << 40, p, p, None) == -3
    assert lib.drn_nms(p, p, -1, 0.5, p, 1 << 40, p, p, None) == -1
    assert lib.drn_nms(p, p, 8, 0.5, p, 16, p, p, None) == -1                 # workspace too small
    assert lib.drn_batched_nms(p, p, None, 8, 0.5, p, 1 << 40, p, p, None) == -1
    assert lib.drn_detect_all(p, p, 26215, 20, 20, 1.0, 1.0, 0.0, 0.5, -1, p, 1 << 40, 524300, p, p, p, p, p, None) == -3
    assert lib.drn_detect_all(p, p, 4, 2, 2, 1.0, 1.0, 0.0, 0.5, 0, p, 1 << 40, 8, p, p, p, p, p, None) == -1
    assert lib.drn_pairwise_iou(None, None, 0, 5, None, None) == 0 and lib.drn_pairwise_iou(None, None, 5, 0, None, None) == 0
    assert lib.drn_pairwise_iou(None, None, 2, 2, None, None) == -1
    th, lb = (ctypes.c_float * 4)(0.1, 0.2, 0.3, 0.4), (ctypes.c_int * 5)(0, 0, 0, 0, 1)
    thp, lbp = ctypes.cast(th, ctypes.c_void_p), ctypes.cast(lb, ctypes.c_void_p)
    assert lib.drn_match(p, 2, 2, thp, 4, lbp, p, p, None) == -3
    bad = (ctypes.c_int * 2)(0, 2)
    assert lib.drn_match(p, 2, 2, thp, 1, ctypes.cast(bad, ctypes.c_void_p), p, p, None) == -1
    assert one.value == 5
    assert lib.drn_detect_all_workspace_bytes(40000) > lib.drn_detect_workspace_bytes(40000)
    # linear in cap as well
    f = lib.drn_detect_all_workspace_bytes
    assert (f(1 << 15) - f(1 << 14)) * 2 == f(1 << 16) - f(1 << 15)


def test_matcher_still_refuses_low_quality_matches(pkg):
    rh = importlib.import_module("drn_wsod_pytorch_amd.modeling.roi_heads")
    with pytest.raises(pkg._cabi.DrnError):
        rh.Matcher([0.5], [0, 1], allow_low_quality_matches=True)
    m = rh.Matcher([0.1, 0.5], [-1, 0, 1])
    assert callable(m) and m.thresholds[1:-1] == [0.1, 0.5]


def test_generator_cases_can_fail():
    """what the GPU tests rely on, checked where the oracle alone is needed: the kept share, the revived boxes (asserted inside
    checked_case) and the hand-made expectations"""
    for n in (63, 65, 129, U.PANEL + 1):
        for thr in (0.3, 0.5, 0.7):
            c = U.checked_case(n, thr)
            assert 0 < len(c["keep"]) < n
    for thr in (0.3, 0.5, 0.7):
        c = U.checked_case(129, thr, 20)
        assert c["classes"].dtype == torch.int64 and int(c["classes"].max()) == 19
    # revived boxes also at n = 65 for the two lower thresholds
    for thr in (0.3, 0.5):
        c = U.checked_case(65, thr)
        assert U.revived_count(c["boxes"].numpy(), c["scores"].numpy(), None, c["keep"].numpy(), thr) >= 1
