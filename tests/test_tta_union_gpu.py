"""GPU tests of GeneralizedRCNNWithTTAUNION: ops.detect_union_batch (csrc/detect.hip: union_count_kernel / union_place_kernel in
front of the batched tail's own sort / NMS / gather) against the merged detections the reference produced, and against the numpy
restatement of tests/tta_union_util.py (pinned to that golden by test_tta_union_cpu.py) at the kernels' edges; the wrapper on the
tiny model; the dataset loop.  The op is compared bit for bit: it gets the same input bits as the helper, performs the reference's
float32 operations in their order and integer bookkeeping - there is no tolerance to choose.  The wrapper's final detections are
compared with the reference's within the bounds test_tta_matches_reference_golden uses for this model in fp32 (scores rtol 1e-4 /
atol 1e-6, boxes rtol 1e-5 / atol 1e-3), for the runs whose NMS / score margins the golden's generator asserts."""
import numpy as np
import pytest
import torch

import golden_util as G
import tta_union_util as U
from __graft_entry__ import load_package

pytestmark = pytest.mark.gpu
load_package()
from drn_wsod_pytorch_amd import evaluation as E  # noqa: E402
from drn_wsod_pytorch_amd import ops  # noqa: E402
from drn_wsod_pytorch_amd import _cabi as C  # noqa: E402
from drn_wsod_pytorch_amd._cabi import DrnError  # noqa: E402
from drn_wsod_pytorch_amd.modeling import DatasetMapperTTAAVG, DatasetMapperTTAUNION, GeneralizedRCNNWithTTAUNION  # noqa: E402
from drn_wsod_pytorch_amd.structures import Boxes, DetectionBatch, Instances  # noqa: E402

DEV = "cuda"


def bits(t):
    return t.contiguous().view(torch.int32)


def garbage_out(n_img, topk):
    return (torch.full((n_img, topk, 4), float("nan"), device=DEV), torch.full((n_img, topk), -7.5, device=DEV),
            torch.full((n_img, topk), 1234, dtype=torch.int32, device=DEV), torch.full((n_img, topk), 4321, dtype=torch.int32, device=DEV),
            torch.full((n_img,), 99, dtype=torch.int32, device=DEV))


def raw_union(dev, img_off, tfms, sizes, K, nms, topk, out):
    """drn_detect_union_batch through the C ABI into the caller's own output buffers (ops.detect_union_batch allocates its own)"""
    import ctypes

    boxes, scores, classes, count = dev
    B, T = scores.shape
    n_img = len(sizes)
    nbytes = C.lib().drn_detect_union_workspace_bytes(B * T, n_img)
    ws = torch.empty((nbytes,), dtype=torch.uint8, device=DEV)
    tfm = [v for sx, sy, fw in tfms for v in (np.float32(sx), np.float32(sy), fw)]
    geom = [v for hw in sizes for v in hw]
    hp = lambda a: ctypes.cast(a, ctypes.c_void_p)
    C.call("drn_detect_union_batch", C.ptr(boxes), C.ptr(scores), C.ptr(classes), C.ptr(count), B, T, hp(C.host_ints(img_off)), n_img,
           hp(C.host_floats(tfm)), hp(C.host_floats(geom)), K, 1e-8, float(nms), topk, C.ptr(ws), nbytes, B * T,
           *[C.ptr(t) for t in out], C.stream())
    return out


def run_op(bb, bs, bc, cnt, img_off, tfms, sizes, K, nms, topk):
    """ops.detect_union_batch, then the entry itself into outputs pre-filled with garbage: the same bits - the buffers must be a
    function of the inputs alone"""
    dev = [torch.from_numpy(np.ascontiguousarray(a)).to(DEV) for a in (bb, bs, bc, cnt)]
    first = [t.cpu() for t in ops.detect_union_batch(*dev, img_off, tfms, sizes, num_classes=K, nms_thresh=nms, topk=topk)]
    got = [t.cpu() for t in raw_union(dev, img_off, tfms, sizes, K, nms, topk, garbage_out(len(sizes), topk))]
    for a, b in zip(first, got):
        assert a.dtype == b.dtype and torch.equal(bits(a), bits(b))
    return got


def check_against_helper(got, bb, bs, bc, cnt, img_off, tfms, sizes, K, nms, topk):
    ob, os_, oc, orow, ocnt = got
    N = len(sizes)
    assert ob.shape == (N, topk, 4) and os_.shape == oc.shape == orow.shape == (N, topk) and ocnt.shape == (N,)
    kept = []
    for i in range(N):
        b0, b1 = img_off[i], img_off[i + 1]
        if b1 > b0:
            ub, us, uc = U.union_rows(bb[b0:b1], bs[b0:b1], bc[b0:b1], cnt[b0:b1], tfms[b0:b1])
        else:
            ub, us, uc = np.zeros((0, 4), np.float32), np.zeros((0,), np.float32), np.zeros((0,), np.int64)
        rb, rs, rc, rr = U.merge(ub, us, uc, sizes[i], K, nms, topk)
        n = int(ocnt[i])
        print("image %d: %d union rows, %d merged (helper %d)" % (i, len(us), n, len(rs)))
        assert n == len(rs), (i, n, len(rs))
        assert np.array_equal(oc[i, :n].numpy(), rc) and np.array_equal(orow[i, :n].numpy(), rr), i
        assert np.array_equal(os_[i, :n].numpy().view(np.int32), rs.view(np.int32)), i
        assert np.array_equal(ob[i, :n].numpy().view(np.int32), np.ascontiguousarray(rb).view(np.int32)), i
        assert not bits(ob[i, n:]).any() and not bits(os_[i, n:]).any(), i  # the fill: +0.0 / +0.0 / -1 / -1
        assert bool((oc[i, n:] == -1).all()) and bool((orow[i, n:] == -1).all()), i
        kept.append((rb, rs, rc, rr, len(us)))
    return kept


# ---- 1. the op against the reference ---------------------------------------------------------------------------------------

@pytest.mark.parametrize("tag,topk", U.CASES)
def test_op_matches_reference_golden(tag, topk):
    d = G.load("tta_union_r50c4_tiny")
    pre = "%s_k%d_" % (tag, topk)
    bb, bs, bc, cnt, tfms = U.golden_blocks(d, tag, topk)
    H, W = d["image_u8"].shape[1:]
    ob, os_, oc, orow, ocnt = run_op(bb, bs, bc, cnt, [0, len(cnt)], tfms, [(H, W)], int(d["num_classes"]), float(d["nms_thresh"]),
                                     topk)
    n = int(ocnt[0])
    assert n == len(d[pre + "det_scores"]) > 0
    assert np.array_equal(oc[0, :n].numpy(), d[pre + "det_classes"])
    assert np.array_equal(os_[0, :n].numpy().view(np.int32), d[pre + "det_scores"].view(np.int32))
    assert np.array_equal(ob[0, :n].numpy().view(np.int32), d[pre + "det_boxes"].view(np.int32))
    assert np.array_equal(orow[0, :n].numpy(), d[pre + "det_rows"])  # the union rows the reference's own function kept
    assert np.array_equal(d[pre + "union_scores"][orow[0, :n].numpy()], d[pre + "det_scores"])
    assert not bits(ob[0, n:]).any() and not bits(os_[0, n:]).any() and bool((oc[0, n:] == -1).all())


# ---- 2. the op against the helper at the kernels' edges ----------------------------------------------------------------------

K3 = 3


def make_case(n_images, n_blocks, blk_topk, seed, all_live=False, lead_empty=0):
    """random padded blocks in the augmented images' coordinates with the edge material of the issue in LIVE slots; lead_empty: that
    many images at the front have no block at all"""
    rs = np.random.RandomState(seed)
    T = blk_topk
    # blocks per image: spread unevenly; with images to spare, image 3 has no block at all
    edges = np.linspace(0, n_blocks, n_images - lead_empty + 1).astype(np.int64)
    if n_images - lead_empty >= 5:
        edges[4] = edges[3]
    img_off = [0] * lead_empty + [int(e) for e in edges]
    sizes = [(60 + 7 * (i % 5), 84 + 5 * (i % 3)) for i in range(n_images)]
    menu = [0, 1, 63, 64, 65, T]
    cnt = np.array([min(menu[(b + seed) % len(menu)], T) for b in range(n_blocks)], np.int32)
    if all_live:
        cnt[:] = T
    else:
        cnt[0] = 0            # an empty block first,
        cnt[n_blocks // 2] = 0  # in the middle
        cnt[-1] = 0           # and last
        if n_blocks > 4:
            cnt[1] = T + 5    # a count beyond the capacity is held to it
        if n_images >= 3:
            cnt[img_off[1]: img_off[2]] = 0  # an image whose blocks are all empty
    bb = np.zeros((n_blocks, T, 4), np.float32)
    bs = np.zeros((n_blocks, T), np.float32)
    bc = np.zeros((n_blocks, T), np.int32)
    tfms = []
    for b in range(n_blocks):
        img = max(i for i in range(n_images) if img_off[i] <= b)
        H, W = sizes[img]
        nh, nw = [(48, 67), (72, 101), (61, 85), (96, 134)][b % 4]
        fl = b % 2 == 1  # flipped and unflipped blocks
        tfms.append((W * 1.0 / nw, H * 1.0 / nh, float(nw) if fl else -1.0))
        x0, y0 = rs.uniform(-12, nw * 0.9, T), rs.uniform(-12, nh * 0.9, T)  # some leave the image after the back-transform
        bb[b] = np.stack([x0, y0, x0 + rs.uniform(2, nw * 0.7, T), y0 + rs.uniform(2, nh * 0.7, T)], 1)
        bs[b] = np.ceil(rs.uniform(0.0, 1.0, T) * 16) / 16  # 16 levels: equal scores within and across blocks
        bc[b] = rs.randint(0, K3, T)
        n = min(int(cnt[b]), T)
        if n >= 60:
            bs[b, 3] = np.float32(1e-8)                                   # at the threshold: no candidate, still a row
            bs[b, 4] = np.nextafter(np.float32(1e-8), np.float32(0))      # below
            bs[b, 5] = np.nextafter(np.float32(1e-8), np.float32(1))      # just above: a candidate
            bs[b, 6] = 0.0
            bb[b, 9, 2] = np.nan                                          # a NaN box and an inf score: rows dropped, numbering compacts
            bs[b, 11] = np.inf
            bb[b, 13] = [nw + 30.0, 5.0, nw + 60.0, 20.0]                 # wholly outside: clipped to zero width on the border
    return bb, bs, bc, cnt, img_off, tfms, sizes


def poison_beyond_count(bb, bs, bc, cnt):
    bb, bs, bc = bb.copy(), bs.copy(), bc.copy()
    T = bs.shape[1]
    for b in range(bs.shape[0]):
        n = min(max(int(cnt[b]), 0), T)
        bb[b, n:] = np.nan
        bs[b, n:] = 1e30
        bc[b, n:] = 99
        if n + 1 < T:
            bs[b, n + 1] = np.nan
    return bb, bs, bc


@pytest.mark.parametrize("n_images,n_blocks,blk_topk,topk,all_live", [
    (1, 1, 1, 1, True),         # the smallest call
    (1, 1, 1, 100, False),      # one block, and it is empty
    (3, 16, 64, 100, False),    # a wave's worth of slots per block
    (3, 17, 65, 100, False),    # one slot / one block more
    (1, 16, 100, 100, True),    # 1600 candidates, far more than topk
    (1, 16, 100, 1, True),
    (16, 17, 64, 100, False),   # sixteen images, some without any block
    (16, 256, 100, 1024, False),
    (3, 256, 1, 1024, False),
])
def test_op_matches_helper_at_the_edges(n_images, n_blocks, blk_topk, topk, all_live):
    bb, bs, bc, cnt, img_off, tfms, sizes = make_case(n_images, n_blocks, blk_topk, 100 + n_blocks + blk_topk, all_live)
    nms = 0.4
    got = run_op(bb, bs, bc, cnt, img_off, tfms, sizes, K3, nms, topk)
    kept = check_against_helper(got, bb, bs, bc, cnt, img_off, tfms, sizes, K3, nms, topk)
    if n_blocks == 1 and not all_live:
        assert int(got[4][0]) == 0
    if all_live and topk == 1:
        assert int(got[4][0]) == 1
    if (n_images, n_blocks) == (1, 16) and topk == 100:
        assert int(got[4][0]) == 100 and kept[0][4] == 1600  # the top-k cut
    if n_images == 3 and n_blocks >= 16 and blk_topk > 1:
        assert int(got[4][1]) == 0 and int(got[4][0]) > 0  # the image whose blocks are all empty
        assert kept[0][4] > 16  # more union rows than score levels: ties, whose order is the union order
    # whatever lies beyond a block's count is never read: NaN / 1e30 / class 99 there change no bit of the result
    pb, ps, pc = poison_beyond_count(bb, bs, bc, cnt)
    again = run_op(pb, ps, pc, cnt, img_off, tfms, sizes, K3, nms, topk)
    for a, b in zip(got, again):
        assert torch.equal(bits(a), bits(b))


def test_op_with_leading_and_adjacent_images_without_blocks():
    """img_off = [0, 0, 0, 8, 16]: the first image has no block and neither has its neighbour - block 0 opens three segments"""
    bb, bs, bc, cnt, img_off, tfms, sizes = make_case(4, 16, 64, 77, lead_empty=2)
    assert img_off == [0, 0, 0, 8, 16]
    got = run_op(bb, bs, bc, cnt, img_off, tfms, sizes, K3, 0.4, 100)
    check_against_helper(got, bb, bs, bc, cnt, img_off, tfms, sizes, K3, 0.4, 100)
    assert got[4].tolist()[:2] == [0, 0] and int(got[4][2]) > 0 and int(got[4][3]) > 0


# ---- 3. the limits ---------------------------------------------------------------------------------------------------------

def test_limits_are_refused_and_leave_the_outputs_untouched():
    """on the host by ops (before any buffer or launch), and by the library itself with the caller's outputs untouched"""
    def attempt(B=2, T=5, n_img=1, topk=10, off=None):  # refused on the host: no output buffer exists yet, nothing is launched
        z = lambda *s, dt=torch.float32: torch.zeros(s, dtype=dt, device=DEV)
        off = [0] + [B] * n_img if off is None else off
        with pytest.raises(DrnError):
            ops.detect_union_batch(z(B, T, 4), z(B, T), z(B, T, dt=torch.int32), z(B, dt=torch.int32), off, [(1.0, 1.0, -1.0)] * B,
                                   [(8, 8)] * n_img, num_classes=3, nms_thresh=0.3, topk=topk)

    attempt(n_img=17)
    attempt(B=257)
    attempt(T=1025)
    attempt(topk=1025)
    attempt(topk=0)
    attempt(off=torch.tensor([0, 2], dtype=torch.int32, device=DEV))  # img_off on the device would need a read-back
    # the library itself answers DRN_ERR_UNSUPPORTED (-3) before any launch
    B, T, topk = 2, 5, 10
    z = lambda *s, dt=torch.float32: torch.zeros(s, dtype=dt, device=DEV)
    ins = (z(B, T, 4), z(B, T), z(B, T, dt=torch.int32), z(B, dt=torch.int32))
    nbytes = C.lib().drn_detect_union_workspace_bytes(B * T, 1)
    ws = torch.empty((nbytes,), dtype=torch.uint8, device=DEV)
    import ctypes

    off17 = C.host_ints([0] + [B] * 17)
    tf = C.host_floats([1.0, 1.0, -1.0] * 300)
    geom = C.host_floats([8.0, 8.0] * 17)
    hp = lambda a: ctypes.cast(a, ctypes.c_void_p)
    for n_blocks, blk_topk, n_images, tk in ((B, T, 17, topk), (B, T, 0, topk), (257, T, 1, topk), (0, T, 1, topk), (B, 1025, 1, topk),
                                             (B, 0, 1, topk), (B, T, 1, 1025), (B, T, 1, 0)):
        out = garbage_out(1, topk)
        keep = [t.clone() for t in out]
        rc = C.lib().drn_detect_union_batch(*[C.ptr(t) for t in ins], n_blocks, blk_topk, hp(off17), n_images, hp(tf), hp(geom), 3,
                                            1e-8, 0.3, tk, C.ptr(ws), nbytes, B * T, *[C.ptr(t) for t in out], C.stream())
        assert rc == -3, (n_blocks, blk_topk, n_images, tk, rc)
        torch.cuda.synchronize()
        for a, b in zip(out, keep):
            assert torch.equal(bits(a), bits(b))


# ---- 4. the wrapper on the tiny model -------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def tiny():
    d = G.load("tta_union_r50c4_tiny")
    ocfg = G.MODEL_CASES["model_r50c4_tiny"]
    cfg, model = G.drn_model(ocfg, int(d["seed"]), "cuda", 5, "fp32")
    model.eval()
    yield d, ocfg, cfg, model
    load_package().set_precision("fp32")


def golden_input(d, image_id=None):
    img = torch.from_numpy(d["image_u8"])
    H, W = img.shape[1:]
    prop = Instances((H, W))
    prop.proposal_boxes = Boxes(torch.from_numpy(d["proposal_boxes"]))
    prop.objectness_logits = torch.from_numpy(d["objectness_logits"])
    inp = {"image": img, "proposals": prop, "height": H, "width": W}
    if image_id is not None:
        inp["image_id"] = image_id
    return inp


def make_mapper(tag, cfg, device):
    return (DatasetMapperTTAAVG if tag == "avg" else DatasetMapperTTAUNION)(cfg, device=device)


@pytest.mark.parametrize("tag,topk", U.CASES)
def test_wrapper_on_the_tiny_model(tiny, tag, topk):
    d, ocfg, cfg, model = tiny
    cfg = cfg.clone()
    cfg.merge_from_list(U.tta_cfg_opts(d, topk))
    pre = "%s_k%d_" % (tag, topk)
    inp = golden_input(d)
    H, W = inp["height"], inp["width"]
    K, nms = cfg.MODEL.ROI_HEADS.NUM_CLASSES, cfg.MODEL.ROI_HEADS.NMS_THRESH_TEST
    assert K == int(d["num_classes"]) and nms == float(d["nms_thresh"]) and cfg.MODEL.ROI_HEADS.SCORE_THRESH_TEST == float(d["score_thresh"])
    default = GeneralizedRCNNWithTTAUNION(cfg, model)
    assert type(default.tta_mapper) is DatasetMapperTTAUNION and default.tta_mapper.device is not None
    for where in ("device", "host"):
        mapper = make_mapper(tag, cfg, model.device if where == "device" else None)
        augs = mapper(inp)
        assert len(augs) == int(d["n_aug"])
        for i, a in enumerate(augs):  # the augmented images (and proposals) are the reference's, bit for bit
            assert a["image"].is_cuda == (where == "device")
            assert np.array_equal(a["image"].cpu().numpy().astype(np.float32), d["aug%d_image" % i].astype(np.float32)), i
            assert np.array_equal(a["proposals"].proposal_boxes.tensor.cpu().numpy(), d[pre + "aug%d_boxes" % i]), i
            assert tuple(a["proposals"].image_size) == tuple(int(v) for v in d[pre + "aug%d_size" % i])
        tta = GeneralizedRCNNWithTTAUNION(cfg, model, tta_mapper=mapper)
        with torch.no_grad():
            det, tfms = tta._get_augmented_detections(augs)
        assert isinstance(det, DetectionBatch) and len(det) == len(augs) and det.topk == topk
        out = tta([inp])[0]["instances"]
        n = len(out)
        assert n > 0 and out.image_size == (H, W) and out.pred_classes.dtype == torch.int64
        # = the op on the wrapper's own per-pass padded detections, bit for bit
        ob, os_, oc, orow, ocnt = ops.detect_union_batch(det.boxes, det.scores, det.classes, det.count, [0, len(det)], tfms, [(H, W)],
                                                         num_classes=K, nms_thresh=nms, topk=topk)
        assert int(ocnt[0]) == n
        assert torch.equal(bits(out.pred_boxes.tensor), bits(ob[0, :n])) and torch.equal(bits(out.scores), bits(os_[0, :n]))
        assert torch.equal(out.pred_classes, oc[0, :n].long())
        # = the numpy helper on those detections read back
        hb, hs, hc, hr = U.merge(*U.union_rows(det.boxes.cpu().numpy(), det.scores.cpu().numpy(), det.classes.cpu().numpy(),
                                               det.count.cpu().numpy(), tfms), (H, W), K, nms, topk)
        assert np.array_equal(out.pred_classes.cpu().numpy(), hc) and np.array_equal(orow[0, :n].cpu().numpy(), hr)
        assert np.array_equal(out.scores.cpu().numpy(), hs) and np.array_equal(out.pred_boxes.tensor.cpu().numpy(), hb)
        # padded=True: the same slots, and a DetectionBatch on the original image size
        pad = GeneralizedRCNNWithTTAUNION(cfg, model, tta_mapper=mapper, padded=True)([inp])
        assert isinstance(pad, DetectionBatch) and pad.image_sizes == [(H, W)] and pad.topk == topk
        for a, b in zip((pad.boxes, pad.scores, pad.classes, pad.rows, pad.count), (ob, os_, oc, orow, ocnt)):
            assert torch.equal(bits(a), bits(b))
        # batch_size = 2: each size's plain and flipped image in one model.inference.  Both mappers: the output is the op on that
        # wrapper's OWN per-pass detections bit for bit, and agrees with batch_size = 1 within the AVG test's bounds
        tta2 = GeneralizedRCNNWithTTAUNION(cfg, model, tta_mapper=mapper, batch_size=2)
        with torch.no_grad():
            det2, tfms2 = tta2._get_augmented_detections(mapper(inp))
        out2 = tta2([inp])[0]["instances"]
        assert tfms2 == tfms
        ob2, os2, oc2, _, ocnt2 = ops.detect_union_batch(det2.boxes, det2.scores, det2.classes, det2.count, [0, len(det2)], tfms2,
                                                         [(H, W)], num_classes=K, nms_thresh=nms, topk=topk)
        n2 = int(ocnt2[0])
        assert n2 == len(out2) and torch.equal(bits(out2.pred_boxes.tensor), bits(ob2[0, :n2]))
        assert torch.equal(bits(out2.scores), bits(os2[0, :n2])) and torch.equal(out2.pred_classes, oc2[0, :n2].long())
        c1, c2 = out.pred_classes.cpu().numpy(), out2.pred_classes.cpu().numpy()
        s1, s2 = out.scores.cpu().numpy(), out2.scores.cpu().numpy()
        b1, b2 = out.pred_boxes.tensor.cpu().numpy(), out2.pred_boxes.tensor.cpu().numpy()
        print("%s %s batch_size 2 vs 1: %d vs %d detections" % (pre, where, n2, n), end="")
        if n2 == n:
            print(", classes equal %s, max |dscore| %.3g, max |dbox| %.3g" % (np.array_equal(c1, c2), np.abs(s1 - s2).max(),
                                                                             np.abs(b1 - b2).max()))
        assert n2 == n and np.array_equal(c2, c1)
        assert np.allclose(s2, s1, rtol=1e-4, atol=1e-6) and np.allclose(b2, b1, rtol=1e-5, atol=1e-3)
        if tag == "avg":
            # the final detections against the reference's (the generator asserts this run's margins)
            assert np.array_equal(c1, d[pre + "det_classes"])
            assert np.allclose(s1, d[pre + "det_scores"], rtol=1e-4, atol=1e-6)
            assert np.allclose(b1, d[pre + "det_boxes"], rtol=1e-5, atol=1e-3)


def test_refuses_masks_and_keypoints(tiny):
    d, ocfg, cfg, model = tiny
    for key in ("MODEL.MASK_ON", "MODEL.KEYPOINT_ON"):
        bad = cfg.clone()
        bad.merge_from_list([key, "True"])
        with pytest.raises((DrnError, AssertionError)):
            GeneralizedRCNNWithTTAUNION(bad, model)


# ---- 5. through the dataset loop -------------------------------------------------------------------------------------------

def test_through_the_dataset_loop(tiny):
    d, ocfg, cfg, model = tiny
    cfg = cfg.clone()
    cfg.merge_from_list(U.tta_cfg_opts(d, 100))
    base = golden_input(d)
    H, W = base["height"], base["width"]
    inputs = []
    for i in range(3):
        prop = Instances((H, W))
        prop.proposal_boxes = Boxes(torch.from_numpy(d["proposal_boxes"][i::3].copy()))  # different numbers of proposals
        prop.objectness_logits = torch.from_numpy(d["objectness_logits"][i::3].copy())
        im = torch.flip(base["image"], dims=[2]) if i % 2 else base["image"]
        inputs.append({"image": im.contiguous(), "proposals": prop, "height": H, "width": W, "image_id": "%06d" % (i + 1)})
    loader = [[inputs[0]], inputs[1:]]
    names = ["c%d" % i for i in range(ocfg.num_classes)]
    annos = {x["image_id"]: [(names[(i + j) % len(names)], j % 2, [1 + 3 * i, 2 + j, W // 2 + 5 * j, H // 2 + 7 * i])
                             for j in range(3)] for i, x in enumerate(inputs)}
    mapper = DatasetMapperTTAAVG(cfg, device=model.device)
    plain = GeneralizedRCNNWithTTAUNION(cfg, model, tta_mapper=mapper)
    ev = E.PascalVOCDetectionEvaluator(names, annotations=annos, year=2007, device="cuda")
    ev.reset()
    for el in loader:
        ev.process(el, plain(el))
    want = ev.evaluate()
    padded = GeneralizedRCNNWithTTAUNION(cfg, model, tta_mapper=mapper, padded=True)
    got = E.inference_on_dataset(padded, loader, E.PascalVOCDetectionEvaluator(names, annotations=annos, year=2007, device="cuda"))

    def flat(r, pre=""):
        out = []
        for k in sorted(r):
            out += flat(r[k], pre + k + "/") if isinstance(r[k], dict) else [(pre + k, r[k])]
        return out

    fa, fb = flat(want), flat(got)
    assert [k for k, _ in fa] == [k for k, _ in fb] and len(fa) > 0
    for (k, x), (_, y) in zip(fa, fb):
        assert x == y or (np.isnan(x) and np.isnan(y)), (k, x, y)
