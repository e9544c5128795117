"""GPU tests of the batched, sync-free inference tail (ops.detect_topk_batch, csrc/detect.hip) and of ops.detections_compact.
The expectation is built per image on the CPU: the oracle's fast_rcnn_inference_single_image, then the package's own
detector_postprocess on CPU Instances.  Everything is compared bit for bit (torch.equal): the tail performs the oracle's single
fp32 operations in its order and integer bookkeeping - there is no tolerance to choose.  Every case runs twice and the two
results, fill included, must have the same bits."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import golden_util as G
from __graft_entry__ import load_package

pytestmark = pytest.mark.gpu
O = G.O
load_package()
from drn_wsod_pytorch_amd import ops  # noqa: E402
from drn_wsod_pytorch_amd._cabi import DrnError  # noqa: E402
from drn_wsod_pytorch_amd.modeling.rcnn import detector_postprocess  # noqa: E402
from drn_wsod_pytorch_amd.structures import Boxes, Instances  # noqa: E402

DEV = "cuda"


def make_image(R, K, seed, size, levels=0, scale=2.0):
    """boxes [R, 4K] decoded from random deltas around random proposals (some leave the image), softmax scores [R, K+1]"""
    rs = np.random.RandomState(seed)
    h, w = size
    x0, y0 = rs.uniform(-10, w * 0.8, R), rs.uniform(-10, h * 0.8, R)
    props = np.stack([x0, y0, x0 + rs.uniform(4, w * 0.6, R), y0 + rs.uniform(4, h * 0.6, R)], 1).astype(np.float32)
    boxes = O.apply_deltas(torch.from_numpy(rs.standard_normal((R, 4 * K)).astype(np.float32) * 0.5), torch.from_numpy(props))
    scores = F.softmax(torch.from_numpy(rs.standard_normal((R, K + 1)).astype(np.float32) * scale), 1)
    if levels:
        scores = (scores * levels).ceil() / levels
    return boxes.contiguous(), scores.contiguous()


def expect_image(boxes, scores, size, out_size, thr, nms, topk):
    rb, rs_, rc, rr = O.fast_rcnn_inference_single_image(boxes.clone(), scores.clone(), size, thr, nms, topk)
    if out_size is None:
        return rb, rs_, rc, rr
    inst = detector_postprocess(Instances(size, pred_boxes=Boxes(rb), scores=rs_, pred_classes=rc, rows=rr), *out_size)
    return inst.pred_boxes.tensor, inst.scores, inst.pred_classes, inst.rows


def run_batch(images, sizes, out_sizes, thr, nms, topk):
    off = [0]
    for b, _ in images:
        off.append(off[-1] + b.shape[0])
    boxes, scores = torch.cat([b for b, _ in images]).to(DEV), torch.cat([s for _, s in images]).to(DEV)
    first = None
    for _ in range(2):  # twice: the result may not depend on how the workgroups were scheduled
        got = [t.cpu() for t in ops.detect_topk_batch(boxes, scores, off, sizes, out_sizes, score_thresh=thr, nms_thresh=nms,
                                                      topk=topk)]
        if first is None:
            first = got
        else:
            for a, b in zip(first, got):
                assert a.dtype == b.dtype and torch.equal(a.view(torch.int32), b.view(torch.int32))
    return first


def check_batch(images, sizes, out_sizes, thr=1e-5, nms=0.3, topk=100):
    ob, os_, oc, orow, cnt = run_batch(images, sizes, out_sizes, thr, nms, topk)
    N = len(images)
    assert ob.shape == (N, topk, 4) and os_.shape == (N, topk) and oc.shape == (N, topk) and orow.shape == (N, topk)
    assert cnt.shape == (N,) and oc.dtype == torch.int32 and orow.dtype == torch.int32 and cnt.dtype == torch.int32
    want = []
    for i, (b, s) in enumerate(images):
        eb, es, ec, er = expect_image(b, s, sizes[i], None if out_sizes is None else out_sizes[i], thr, nms, topk)
        n = int(cnt[i])
        print("image %d: %d detections (oracle %d)" % (i, n, es.shape[0]))
        assert n == es.shape[0], (i, n, es.shape[0])
        assert torch.equal(orow[i, :n].long(), er) and torch.equal(oc[i, :n].long(), ec), i
        assert torch.equal(os_[i, :n], es) and torch.equal(ob[i, :n], eb), i
        # the fill beyond the count: the buffers are a function of the inputs alone
        assert not ob[i, n:].any() and not os_[i, n:].any(), i
        assert bool((oc[i, n:] == -1).all()) and bool((orow[i, n:] == -1).all()), i
        want.append((eb, es, ec, er))
    return want


def test_mixed_batch():
    """N = 3, R = (130, 1, 70), K = 20: image 0's 2600 entries cross a 2048-entry compaction tile and the tile that ends it runs
    into image 1; image 2 is all background (count 0); one row of image 0 is non-finite (rows are renumbered per image);
    different (h, w) per image, output sizes with non-dyadic ratios"""
    sizes = [(150, 200), (90, 120), (111, 77)]
    outs = [(337, 451), (95, 131), (200, 150)]
    imgs = [make_image(130, 20, 1, sizes[0]), make_image(1, 20, 2, sizes[1]), make_image(70, 20, 3, sizes[2])]
    imgs[0][0][17, 3] = float("inf")
    imgs[2][1].zero_()
    imgs[2][1][:, -1] = 1.0
    want = check_batch(imgs, sizes, outs)
    assert want[2][1].numel() == 0 and want[0][1].numel() > 0 and want[1][1].numel() > 0
    assert int(want[0][3].max()) <= 128  # 129 finite rows
    check_batch(imgs, sizes, None)  # the raw tail


def test_ties_across_the_image_boundary():
    """scores quantised to 4 levels in two images: only the stable order by candidate index, restarting per image, gives the
    oracle's rows"""
    sizes = [(150, 200), (120, 160)]
    imgs = [make_image(90, 20, 11, sizes[0], levels=4), make_image(110, 20, 12, sizes[1], levels=4)]
    assert len(torch.unique(torch.cat([s for _, s in imgs]))) <= 5
    check_batch(imgs, sizes, [(300, 333), (77, 201)])


def test_per_image_branch_and_offset():
    """R = (2100, 300), K = 20, every score above the threshold: image 0's 42 000 candidates take batched_nms's per-class branch,
    image 1's 6 000 the offset branch with its own largest coordinate"""
    sizes = [(150, 200), (300, 420)]
    imgs = [make_image(2100, 20, 21, sizes[0]), make_image(300, 20, 22, sizes[1])]
    assert [int((s[:, :-1] > 0.0).sum()) for _, s in imgs] == [42000, 6000]
    check_batch(imgs, sizes, [(200, 150), (299, 431)], thr=0.0)


@pytest.mark.parametrize("topk", [100, 7])
def test_early_exit_in_one_image_and_fewer_in_another(topk):
    sizes = [(150, 200), (90, 120)]
    imgs = [make_image(130, 20, 31, sizes[0]), make_image(1, 20, 32, sizes[1])]
    imgs[1][1].zero_()
    imgs[1][1][0, :3] = torch.tensor([0.3, 0.2, 0.1])
    imgs[1][1][0, -1] = 0.4
    want = check_batch(imgs, sizes, None, topk=topk)
    assert want[0][1].numel() == topk and want[1][1].numel() == 3


def test_box_dropped_by_the_postprocess():
    """a high-scoring box entirely outside the image survives the NMS (clipped to zero width on the border, it overlaps nothing)
    and is dropped by the postprocess from the middle of the list: later detections move up, the count drops by one"""
    sizes = [(150, 200), (90, 120)]
    imgs = [make_image(60, 20, 41, sizes[0]), make_image(30, 20, 42, sizes[1])]
    b, s = imgs[0]
    b[5] = torch.tensor([230.0, 5.0, 260.0, 40.0]).repeat(20)
    raw = expect_image(b, s, sizes[0], None, 1e-5, 0.3, 100)
    s[5].zero_()
    s[5, 2] = float(raw[1][3]) * 0.999 + float(raw[1][4]) * 0.001  # between the 4th and the 5th detection
    s[5, -1] = 1.0 - float(s[5, 2])
    raw = expect_image(b, s, sizes[0], None, 1e-5, 0.3, 100)
    want = check_batch(imgs, sizes, [(300, 400), (95, 131)])
    at = [i for i in range(raw[3].numel()) if int(raw[3][i]) == 5 and int(raw[2][i]) == 2]
    assert len(at) == 1 and 0 < at[0] < raw[3].numel() - 1
    assert want[0][1].numel() == raw[1].numel() - 1
    assert torch.equal(want[0][3], torch.cat([raw[3][: at[0]], raw[3][at[0] + 1:]]))


def test_single_image_equals_detect_topk():
    size = (150, 200)
    b, s = make_image(500, 20, 51, size)
    got = run_batch([(b, s)], [size], None, 1e-5, 0.3, 100)
    rb, rs_, rc, rr = (t.cpu() for t in ops.detect_topk(b.to(DEV), s.to(DEV), size, 1e-5, 0.3, 100))
    n = int(got[4][0])
    assert n == rs_.shape[0] and n > 0
    assert torch.equal(got[0][0, :n], rb) and torch.equal(got[1][0, :n], rs_)
    assert torch.equal(got[2][0, :n].long(), rc) and torch.equal(got[3][0, :n].long(), rr)


def test_sixteen_tiny_images():
    sizes = [(40 + 3 * i, 50 + 2 * i) for i in range(16)]
    imgs = [make_image(5, 3, 60 + i, sizes[i]) for i in range(16)]
    check_batch(imgs, sizes, [(h + 7, w * 2 - 3) for h, w in sizes])


def test_limits_are_refused_on_the_host():
    size = (40, 50)
    imgs = [make_image(2, 3, 70 + i, size) for i in range(ops.DETECT_MAX_IMAGES + 1)]
    boxes, scores = torch.cat([b for b, _ in imgs]).to(DEV), torch.cat([s for _, s in imgs]).to(DEV)
    with pytest.raises(DrnError):
        ops.detect_topk_batch(boxes, scores, list(range(0, 2 * len(imgs) + 1, 2)), [size] * len(imgs), None, score_thresh=1e-5,
                              nms_thresh=0.3, topk=100)
    M, K = ops.DETECT_BATCH_MAX_ENTRIES // 20 + 1, 20
    with pytest.raises(DrnError):
        ops.detect_topk_batch(torch.zeros((M, 4), device=DEV), torch.zeros((M, K + 1), device=DEV), [0, M], [size], None,
                              score_thresh=1e-5, nms_thresh=0.3, topk=100)
    with pytest.raises(DrnError):
        ops.detect_topk_batch(boxes, scores, torch.tensor([0, boxes.shape[0]], dtype=torch.int32, device=DEV), [size], None,
                              score_thresh=1e-5, nms_thresh=0.3, topk=100)  # img_off on the device would need a read-back


def test_detections_compact():
    rs = np.random.RandomState(81)
    B, topk = 5, 100
    count = torch.tensor([0, 100, 3, 0, 7], dtype=torch.int32)
    image = torch.tensor([4, 2, 9, 1, 2], dtype=torch.int32)
    boxes = torch.from_numpy(rs.uniform(0, 300, (B, topk, 4)).astype(np.float32))
    scores = torch.from_numpy(rs.uniform(0, 1, (B, topk)).astype(np.float32))
    classes = torch.from_numpy(rs.randint(0, 20, (B, topk)).astype(np.int32))
    for _ in range(2):
        ob, os_, oc, oi, n = (t.cpu() for t in ops.detections_compact(boxes.to(DEV), scores.to(DEV), classes.to(DEV),
                                                                      count.to(DEV), image.to(DEV)))
        assert int(n) == 110 and n.dtype == torch.int32
        sl = lambda t: torch.cat([t[b, : int(count[b])] for b in range(B)])
        assert torch.equal(ob[:110], sl(boxes)) and torch.equal(os_[:110], sl(scores)) and torch.equal(oc[:110], sl(classes))
        assert torch.equal(oi[:110], torch.repeat_interleave(image, count.long()))
        assert not ob[110:].any() and not os_[110:].any()
