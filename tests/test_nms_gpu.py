"""GPU tests of the stand-alone box operators (csrc/nms.hip, csrc/boxmatch.hip, drn_detect_all in csrc/detect.hip): nms, batched_nms,
detect_all, pairwise_iou and Matcher.__call__ against the oracle's definitions.  Every comparison is of integers or of float32 bits:
the oracle computes single IEEE fp32 operations and compares, and so do the kernels - there is no tolerance to choose."""
import importlib

import numpy as np
import pytest
import torch

import golden_util as G
import nms_util as U
from __graft_entry__ import load_package
from oracle import wsod_oracle as O

pytestmark = pytest.mark.gpu

THRS = (0.3, 0.5, 0.7)
# 0 .. 129: the 64-bit word edges; 4097: 9 panels, a last panel of one row; PANEL - 1, PANEL, PANEL + 1; 1100: three panels
SIZES = (0, 1, 2, 63, 64, 65, 127, 128, 129, 4097, U.PANEL - 1, U.PANEL, U.PANEL + 1, 2 * U.PANEL + 76)


@pytest.fixture(scope="module")
def ops():
    load_package()
    return importlib.import_module("drn_wsod_pytorch_amd.ops")


def same(got, want):
    got = got.cpu()
    return got.dtype == want.dtype and got.shape == want.shape and torch.equal(got, want)


def bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


@pytest.mark.parametrize("thr", THRS)
@pytest.mark.parametrize("n", SIZES)
def test_nms_equals_oracle(n, thr, ops):
    c = U.checked_case(n, thr)
    b, s = c["boxes"].cuda(), c["scores"].cuda()
    b0, s0 = b.clone(), s.clone()
    got = ops.nms(b, s, thr)
    assert got.is_cuda and same(got, c["keep"])
    keep, count = ops.nms(b, s, thr, padded=True)
    assert keep.dtype == torch.int64 and keep.shape == (n,) and count.dtype == torch.int32 and count.shape == (1,)
    assert int(count) == len(c["keep"]) and same(keep[: int(count)], c["keep"])
    assert torch.equal(b, b0) and torch.equal(s, s0)  # inputs are never written


def test_nms_c_entry_with_no_boxes(ops):
    """n = 0 at the C entry: one store of n_keep = 0, every other pointer may be NULL"""
    C = importlib.import_module("drn_wsod_pytorch_amd._cabi")
    nk = torch.full((1,), 7, dtype=torch.int32, device="cuda")
    C.call("drn_nms", None, None, 0, 0.5, None, 0, None, C.ptr(nk), C.stream())
    assert int(nk) == 0
    nk.fill_(7)
    C.call("drn_batched_nms", None, None, None, 0, 0.5, None, 0, None, C.ptr(nk), C.stream())
    assert int(nk) == 0
    big = ops.NMS_MAX_N + 1
    assert C.lib().drn_nms(None, None, big, 0.5, None, 0, None, C.ptr(nk), C.stream()) == -3  # DRN_ERR_UNSUPPORTED, before any launch


def test_chain_across_a_word_edge(ops):
    """A, B, C at sorted positions 63, 64, 65 behind 63 far-away boxes: IoU(A, B) = 0.8181818, IoU(B, C) = 0.73913044,
    IoU(A, C) = 0.6.  At 0.7 A removes B, and B - removed - must not remove C although its word lies across the edge."""
    far = torch.tensor([[1000.0 + 100.0 * i, 0.0, 1010.0 + 100.0 * i, 10.0] for i in range(63)])
    abc = torch.tensor([[0.0, 0.0, 10.0, 10.0], [1.0, 0.0, 11.0, 10.0], [2.5, 0.0, 12.5, 10.0]])
    boxes = torch.cat([far, abc])
    scores = torch.linspace(0.99, 0.01, 66)
    iou = O.pairwise_iou(abc, abc)
    assert abs(float(iou[0, 1]) - 0.8181818) < 1e-7 and abs(float(iou[1, 2]) - 0.73913044) < 1e-7
    assert abs(float(iou[0, 2]) - 0.6) < 1e-7
    want = O.nms(boxes, scores, 0.7)
    assert want.tolist() == list(range(64)) + [65]
    assert same(ops.nms(boxes.cuda(), scores.cuda(), 0.7), want)
    # the same chain in input order reversed: the sort, not the input order, decides
    perm = torch.arange(65, -1, -1)
    assert same(ops.nms(boxes[perm].cuda(), scores[perm].cuda(), 0.7), O.nms(boxes[perm], scores[perm], 0.7))


def test_threshold_is_strict(ops):
    boxes = torch.tensor([[0.0, 0.0, 2.0, 2.0], [0.0, 0.0, 2.0, 1.0]])
    scores = torch.tensor([0.9, 0.8])
    assert float(O.pairwise_iou(boxes[:1], boxes[1:])) == 0.5
    assert ops.nms(boxes.cuda(), scores.cuda(), 0.5).tolist() == [0, 1] == O.nms(boxes, scores, 0.5).tolist()
    below = float(np.nextafter(np.float32(0.5), np.float32(0)))  # 0.49999997
    assert ops.nms(boxes.cuda(), scores.cuda(), below).tolist() == [0] == O.nms(boxes, scores, below).tolist()


def test_ties_and_degenerate_boxes(ops):
    c = U.checked_case(129, 0.5)
    flat = torch.full((129,), 0.25)
    want = O.nms(c["boxes"], flat, 0.5)
    assert want.tolist() == sorted(want.tolist())  # all scores equal: the order is the input order
    assert same(ops.nms(c["boxes"].cuda(), flat.cuda(), 0.5), want)
    # two scores only, each many times: ties inside every radix digit
    two = torch.where(torch.arange(129) % 3 == 0, torch.tensor(0.75), torch.tensor(0.25))
    assert same(ops.nms(c["boxes"].cuda(), two.cuda(), 0.5), O.nms(c["boxes"], two, 0.5))
    # two identical zero-area boxes: 0 / 0 is NaN, which is not above any threshold - both stay
    z = torch.tensor([[3.0, 4.0, 3.0, 9.0], [3.0, 4.0, 3.0, 9.0]])
    zs = torch.tensor([0.5, 0.6])
    assert O.nms(z, zs, 0.0).tolist() == [1, 0]
    assert ops.nms(z.cuda(), zs.cuda(), 0.0).tolist() == [1, 0]


@pytest.mark.parametrize("n,K,thr", [(129, 20, 0.3), (129, 20, 0.5), (129, 20, 0.7), (39999, 3, 0.5), (40000, 3, 0.5)])
def test_batched_nms_equals_oracle(n, K, thr, ops):
    c = U.checked_case(n, thr, K)
    b, s, i64 = c["boxes"].cuda(), c["scores"].cuda(), c["classes"].cuda()
    assert i64.dtype == torch.int64
    got = ops.batched_nms(b, s, i64, thr)
    assert same(got, c["keep"])
    keep, count = ops.batched_nms(b, s, i64.int(), thr, padded=True)
    assert int(count) == len(c["keep"]) and same(keep[: int(count)], c["keep"])
    assert torch.equal(b.cpu(), c["boxes"]) and torch.equal(s.cpu(), c["scores"]) and torch.equal(i64.cpu(), c["classes"])


def test_batched_nms_negative_coordinates(ops):
    """boxes.max() over boxes that are all negative: the device maximum orders the float bits of negative values as well"""
    c = U.checked_case(129, 0.5, 20)
    b = c["boxes"] - 5000.0
    assert float(b.max()) < 0
    want = O.batched_nms(b, c["scores"], c["classes"], 0.5)
    assert same(ops.batched_nms(b.cuda(), c["scores"].cuda(), c["classes"].cuda(), 0.5), want)


def test_layers_and_structures_surface(ops):
    load_package()
    layers = importlib.import_module("drn_wsod_pytorch_amd.layers")
    structures = importlib.import_module("drn_wsod_pytorch_amd.structures")
    c = U.checked_case(129, 0.5, 20)
    assert same(layers.batched_nms(c["boxes"].cuda(), c["scores"].cuda(), c["classes"].cuda(), 0.5), c["keep"])
    p = U.checked_case(129, 0.5)
    # a double, strided, host-side input is converted
    wide = torch.zeros(129, 8, dtype=torch.float64)
    wide[:, ::2] = p["boxes"].double()
    assert same(layers.nms(wide[:, ::2], p["scores"].double(), 0.5), p["keep"])
    a, b = p["boxes"][:5], p["boxes"][5:70]
    got = structures.pairwise_iou(structures.Boxes(a.cuda()), structures.Boxes(b.cuda()))
    assert torch.equal(bits(got), bits(O.pairwise_iou(a, b)))


# ---- the uncapped tail ------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def tail():
    boxes, scores, hw = U.candidate_set(300, 20)
    return boxes, scores, hw


def check_tail(got, want):
    names = ("boxes", "scores", "classes", "rows")
    for g, w, k in zip(got, want, names):
        g = g.cpu()
        assert g.dtype == w.dtype and g.shape == w.shape, k
        assert torch.equal(bits(g) if g.dtype == torch.float32 else g, bits(w) if w.dtype == torch.float32 else w), k


def test_detect_all_agrees_with_detect_topk(tail, ops):
    boxes, scores, hw = tail
    b, s = boxes.cuda(), scores.cuda()
    b0, s0 = b.clone(), s.clone()
    every = ops.detect_all(b, s, hw, 0.05, 0.5, topk=-1)
    first = ops.detect_topk(b, s, hw, 0.05, 0.5, 100)
    assert len(first[1]) == 100 and len(every[1]) > 1024
    check_tail([t[:100] for t in every], [t.cpu() for t in first])
    check_tail(ops.detect_all(b, s, hw, 0.05, 0.5, topk=100), [t.cpu() for t in first])
    assert torch.equal(bits(b), bits(b0)) and torch.equal(bits(s), bits(s0))


@pytest.mark.parametrize("topk", [-1, 2000])
def test_detect_all_equals_oracle(topk, tail, ops):
    boxes, scores, hw = tail
    every = O.fast_rcnn_inference_single_image(boxes, scores, hw, 0.05, 0.7, -1)
    assert len(every[1]) > 2000  # more survivors than either the one-wave kernel's 1024 or the cut below
    want = O.fast_rcnn_inference_single_image(boxes, scores, hw, 0.05, 0.7, topk)
    assert len(want[1]) == (len(every[1]) if topk < 0 else topk)
    check_tail(ops.detect_all(boxes.cuda(), scores.cuda(), hw, 0.05, 0.7, topk=topk), want)


def test_detect_all_without_candidates(ops):
    boxes, scores = torch.zeros(5, 8).cuda(), torch.zeros(5, 3).cuda()
    got = ops.detect_all(boxes, scores, (10.0, 10.0), 0.05, 0.5)
    assert [len(t) for t in got] == [0, 0, 0, 0]


def test_heads_return_all_detections(monkeypatch, ops):
    """OICRROIHeads with TEST.DETECTIONS_PER_IMAGE -1 returns every survivor (the oracle's count on the very scores and boxes the
    heads handed to the tail); with 100 it goes through detect_topk as before and returns that op's result."""
    name = "model_r50c4_tiny"
    d = G.load(name)
    ocfg = G.MODEL_CASES[name]
    cfg, model = G.drn_model(ocfg, int(d["seed"]), "cuda", 5, "fp32")
    model.eval()
    last = model.roi_heads.box_refinery[-1]
    assert last.test_topk_per_image == cfg.TEST.DETECTIONS_PER_IMAGE == 100
    inputs = G.drn_inputs(G.batch_from(d), with_gt=False)
    seen = []
    real_all, real_topk = ops.detect_all, ops.detect_topk

    def spy(fn, tag):
        def run(b, s, image_shape, score_thresh, nms_thresh, topk):
            out = fn(b, s, image_shape, score_thresh, nms_thresh, topk)
            seen.append((tag, b.clone(), s.clone(), image_shape, score_thresh, nms_thresh, topk, out))
            return out
        return run

    monkeypatch.setattr(ops, "detect_all", spy(real_all, "all"))
    monkeypatch.setattr(ops, "detect_topk", spy(real_topk, "topk"))
    with torch.no_grad():
        out100 = model(inputs)
    assert [t[0] for t in seen] == ["topk"] * len(inputs) and all(t[6] == 100 for t in seen)
    for o, t in zip(out100, seen):
        want = O.fast_rcnn_inference_single_image(t[1].cpu(), t[2].cpu(), t[3], t[4], t[5], 100)
        check_tail(t[7], want)
        assert len(o["instances"]) <= len(want[1])
    del seen[:]
    last.test_topk_per_image = -1
    with torch.no_grad():
        out_all = model(inputs)
    assert [t[0] for t in seen] == ["all"] * len(inputs) and all(t[6] == -1 for t in seen)
    for o, o100, t in zip(out_all, out100, seen):
        want = O.fast_rcnn_inference_single_image(t[1].cpu(), t[2].cpu(), t[3], t[4], t[5], -1)
        check_tail(t[7], want)
        wb = want[0]
        nonempty = int((((wb[:, 2] - wb[:, 0]) > 0) & ((wb[:, 3] - wb[:, 1]) > 0)).sum())
        assert len(o["instances"]) == nonempty >= len(o100["instances"])
    load_package().set_precision("fp32")


# ---- pairwise IoU and Matcher -------------------------------------------------------------------------------------------------
IOU_SHAPES = ((0, 5), (5, 0), (1, 1), (3, 4097), (257, 65))


def iou_inputs(N, M):
    both = U.generate(N + M, 1, seed=11)[0]  # one field for both sets: cluster mates overlap
    a, b = both[:N].copy(), both[N:].copy()
    if N and M:  # a few exact copies of the first two rows: IoU 1, and ties between rows 0 and 1
        a[min(1, N - 1)] = a[0]
        b[:: max(M // 7, 1)] = a[0]
    return torch.from_numpy(a.copy()).reshape(N, 4), torch.from_numpy(b.copy()).reshape(M, 4)


@pytest.mark.parametrize("N,M", IOU_SHAPES)
def test_pairwise_iou_equals_oracle(N, M, ops):
    a, b = iou_inputs(N, M)
    want = O.pairwise_iou(a, b)
    got = ops.pairwise_iou(a.cuda(), b.cuda())
    assert got.shape == (N, M) and got.dtype == torch.float32
    assert torch.equal(bits(got), bits(want))
    if N * M > 64:  # overlapping and disjoint pairs, both
        assert int((want > 0).sum()) > 0 and int((want == 0).sum()) > 0


@pytest.mark.parametrize("thresholds,labels", [([0.5], [0, 1]), ([0.1, 0.5], [-1, 0, 1])])
@pytest.mark.parametrize("N,M", IOU_SHAPES)
def test_matcher_equals_oracle(N, M, thresholds, labels, ops):
    load_package()
    rh = importlib.import_module("drn_wsod_pytorch_amd.modeling.roi_heads")
    a, b = iou_inputs(N, M)
    q = O.pairwise_iou(a, b)
    want = O.matcher(q, tuple(thresholds), tuple(labels))
    m = rh.Matcher(list(thresholds), list(labels), allow_low_quality_matches=False)
    qd = q.cuda()
    q0 = qd.clone()
    got = m(qd)
    for g, w in zip(got, want):
        assert same(g, w)
    assert torch.equal(qd, q0)
    if N and M > 1000:
        assert len(set(want[1].tolist())) == len(labels)  # every interval is hit


def test_matcher_tie_takes_the_first_row(ops):
    load_package()
    rh = importlib.import_module("drn_wsod_pytorch_amd.modeling.roi_heads")
    q = torch.tensor([[0.2, 0.7, 0.0], [0.6, 0.7, 0.0], [0.6, 0.1, 0.0]])
    want = O.matcher(q, (0.5,), (0, 1))
    assert want[0].tolist() == [1, 0, 0] and want[1].tolist() == [1, 1, 0]
    got = rh.Matcher([0.5], [0, 1])(q.cuda())
    assert same(got[0], want[0]) and same(got[1], want[1])


# ---- padded=True: nothing read back, capturable -------------------------------------------------------------------------------
def test_padded_nms_is_capturable(ops):
    n, thr = 4097, 0.5
    cases = [U.checked_case(n, thr, 0, seed) for seed in (1, 2)]
    warm = U.checked_case(n, thr)
    b, s = warm["boxes"].cuda(), warm["scores"].cuda()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        ops.nms(b, s, thr, padded=True)
    torch.cuda.current_stream().wait_stream(side)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):  # a host read inside the capture would fail it
        keep, count = ops.nms(b, s, thr, padded=True)
    for c in cases:
        b.copy_(c["boxes"])
        s.copy_(c["scores"])
        g.replay()
        torch.cuda.synchronize()
        assert int(count) == len(c["keep"]) and same(keep[: int(count)], c["keep"])
