"""The device data path on the GPU: drn_augment_u8 against Pillow and the plain-numpy restatement byte for byte (both of its
paths, every stage on and off, crops flush with the end of the buffer), the device DatasetMapper against the reference's own
output (tests/golden/data_mapper.npz) and against the host mapper at a real size, and the stream contract of
DatasetMapper.finish under GraphedTrainStep's ring schedule and the train loader."""
import numpy as np
import pytest
import torch

import augment_util as A
import golden_util as G
from __graft_entry__ import load_package

pytestmark = pytest.mark.gpu
load_package()
from drn_wsod_pytorch_amd import data as D  # noqa: E402
from drn_wsod_pytorch_amd import ops  # noqa: E402
from drn_wsod_pytorch_amd._cabi import DrnError  # noqa: E402

# name: (H, W), crop (x0, y0, cw, ch) or None = the whole image, (Ho, Wo), staged in LDS (False: the per-pixel path)
KERNEL_CASES = {
    "upscale_odd_offsets": ((37, 53), (5, 3, 41, 29), (64, 91), True),
    "crop_flush_bottom_right": ((37, 53), (12, 8, 41, 29), (64, 91), True),  # the last dword of the buffer is partial
    "downscale_window7": ((120, 160), None, (45, 60), True),
    "no_horizontal_pass": ((50, 60), None, (173, 60), True),
    "no_resize": ((64, 48), None, (64, 48), True),
    "fallback_path": ((600, 800), None, (30, 40), False),
    "real_size": ((375, 500), (30, 20, 450, 340), (800, 1059), True),
}
BLENDS = [(None, None), (1.5, None), (1.5, 1 / 1.5), (1.5, 1.0), (1.5, 1.5)]


def _image(h, w, c, seed):
    """random bytes; the lower half grey (B0 = B1 = B2); a patch of 0 and one of 255 so that both clips fire"""
    rs = np.random.RandomState(seed)
    img = rs.randint(0, 256, (h, w, c)).astype(np.uint8)
    img[h // 2:] = img[h // 2:, :, :1]
    img[h // 4: h // 4 + 6, w // 4: w // 4 + 6] = 0
    img[h // 4: h // 4 + 6, w // 2: w // 2 + 6] = 255
    img[3 * h // 4: 3 * h // 4 + 5, w // 3: w // 3 + 5] = 255
    return img


def _run(img, crop, out_hw, flip, wb, ws):
    h, w = img.shape[:2]
    aug = dict(crop=crop or (0, 0, w, h), out_hw=out_hw, flip=flip, wb=wb, ws=ws)
    got = ops.augment_u8(torch.from_numpy(img).cuda(), crop, out_hw, flip, wb, ws)
    assert got.dtype == torch.float32 and tuple(got.shape) == (img.shape[2],) + tuple(out_hw)
    ref = A.restate(img, aug)
    diff = int((got.cpu().numpy() != ref.astype(np.float32)).sum())
    assert diff == 0, (aug, diff)


@pytest.mark.parametrize("case", list(KERNEL_CASES))
def test_kernel_equals_pillow_and_restatement(case):
    (h, w), crop, out_hw, staged = KERNEL_CASES[case]
    cw, ch = (crop[2], crop[3]) if crop else (w, h)
    assert (ops.augment_u8_lds_bytes((cw, ch), out_hw, 3) > 0) == staged  # which path the launch takes
    img = _image(h, w, 3, 11)
    for flip in (False, True):
        for wb, ws in BLENDS:  # (blends off: the resize alone == Pillow)
            _run(img, crop, out_hw, flip, wb, ws)


@pytest.mark.parametrize("c", [1, 4])
@pytest.mark.parametrize("case", ["upscale_odd_offsets", "crop_flush_bottom_right", "no_resize", "fallback_path"])
def test_kernel_one_and_four_channels(case, c):
    (h, w), crop, out_hw, _ = KERNEL_CASES[case]
    img = _image(h, w, c, 12 + c)
    for flip in (False, True):
        for wb in (None, 1.5):
            _run(img, crop, out_hw, flip, wb, None)


def test_kernel_refusals():
    for c in (1, 4):
        src = torch.from_numpy(_image(20, 30, c, 1)).cuda()
        with pytest.raises(DrnError):
            ops.augment_u8(src, None, (20, 30), False, None, 1.2)  # "RandomSaturation only works on RGB images"
    src = torch.from_numpy(_image(20, 30, 3, 1)).cuda()
    for crop in ((0, 0, 31, 20), (5, 0, 26, 20), (0, 3, 30, 18), (-1, 0, 10, 10), (0, 0, 0, 10)):
        with pytest.raises(DrnError):
            ops.augment_u8(src, crop, (40, 60), False, None, None)
    with pytest.raises(DrnError):
        ops.augment_u8(torch.from_numpy(_image(20, 30, 2, 1)).cuda(), None, (20, 30))
    torch.cuda.synchronize()


def test_device_mapper_equals_reference_golden(tmp_path):
    d, cfg, recs = A.golden_record(tmp_path)
    for tag, is_train, nrep in (("train", True, 4), ("test", False, 1)):
        mapper = D.DatasetMapper(cfg, is_train, device="cuda")
        np.random.seed(int(d["seed"]))
        for rep in range(nrep):
            out = mapper(recs[0])
            k = "%s%d_" % (tag, rep)
            assert "aug" not in out and "image_src" not in out
            im = out["image"]
            assert im.is_cuda and im.dtype == torch.float32
            assert np.array_equal(im.cpu().numpy(), d[k + "image"].astype(np.float32)), k
            A.assert_boxes_equal_golden(out, d, k, is_train)


def test_device_mapper_equals_host_mapper_at_a_real_size():
    """375 x 500 -> short edge 800 with a crop.  The device image equals the restatement exactly; the host mapper forms the
    saturation's grey image with numpy's BLAS dot, whose float64 bits differ from the fixed-order sum in some pixels: an output
    byte can differ only where a float64 value lies within an ulp of an integer - at most 1 PIXEL in 10^5 may differ (a grey value
    shifts the whole pixel), and only by one count."""
    cfg = G.drn_cfg(G.MODEL_CASES["model_r50c4_tiny"], "cpu")
    cfg.merge_from_list(["INPUT.MIN_SIZE_TRAIN", "(800,)", "INPUT.CROP.ENABLED", "True", "MODEL.LOAD_PROPOSALS", "False"])
    img = _image(375, 500, 3, 21)
    rec = {"image_array": img, "height": 375, "width": 500, "image_id": 1}
    host, dev = D.DatasetMapper(cfg, True), D.DatasetMapper(cfg, True, device="cuda")
    for seed in (1, 2, 3):
        np.random.seed(seed)
        a = host(rec)["image"].numpy()
        np.random.seed(seed)
        p = dev.plan(rec)
        b = dev.finish(p)["image"].cpu().numpy()
        assert min(a.shape[1:]) == 800 and a.shape == b.shape
        assert np.array_equal(b, A.restate(img, p["aug"]).astype(np.float32)), seed
        delta = np.abs(a.astype(np.int32) - b.astype(np.int32))
        pixels = int((delta != 0).any(axis=0).sum())
        print("seed %d: %d of %d pixels differ from the host mapper (max %d)" % (seed, pixels, delta[0].size, int(delta.max())))
        assert int(delta.max()) <= 1 and pixels <= delta[0].size // 100000, seed


def _records(n, sizes, n_prop, seed, num_classes):
    rs = np.random.RandomState(seed)
    recs = []
    for i in range(n):
        h, w = sizes[i % len(sizes)]
        x0, y0 = rs.uniform(0, w - 24, n_prop), rs.uniform(0, h - 24, n_prop)
        boxes = np.stack([x0, y0, x0 + rs.uniform(8, 23, n_prop), y0 + rs.uniform(8, 23, n_prop)], 1).astype(np.float32)
        recs.append({"image_array": rs.randint(0, 256, (h, w, 3)).astype(np.uint8), "height": h, "width": w, "image_id": i,
                     "proposal_boxes": boxes, "proposal_objectness_logits": np.sort(rs.rand(n_prop).astype(np.float32))[::-1].copy(),
                     "proposal_bbox_mode": 0,
                     "annotations": [{"bbox": [4.0, 4.0, 30.0, 30.0], "bbox_mode": 0, "category_id": int(rs.randint(num_classes))}]})
    return recs


def test_graphed_ring_steps_fed_by_the_device_loader_equal_the_host_loader():
    """Ordering and lifetime: GraphedTrainStep's ring schedule stages images on a side stream that does not wait for the caller's
    stream, two groups ahead.  Twelve steps fed by build_detection_train_loader(device="cuda") - images produced asynchronously
    on the mapper's stream, two batches in flight - must give the losses of twelve steps fed by the host loader, bit for bit."""
    from drn_wsod_pytorch_amd.engine import GraphedTrainStep, build_optimizer

    name = "model_r50c4_tiny"
    ocfg = G.MODEL_CASES[name]
    seed = int(G.load(name)["seed"])
    recs = _records(6, [(48, 64)], 40, 5, ocfg.num_classes)
    steps, group = 12, 2
    results = []
    for device in (None, "cuda"):
        cfg, model = G.drn_model(ocfg, seed, "cuda", 5, "fp32")
        cfg.merge_from_list(["INPUT.MIN_SIZE_TRAIN", "(64,)", "INPUT.CROP.ENABLED", "False", "SOLVER.IMS_PER_BATCH", "1",
                             "DATALOADER.NUM_WORKERS", "0", "DATASETS.PRECOMPUTED_PROPOSAL_TOPK_TRAIN", "30"])
        model.roi_heads.box_head.dropout_p = 0.0
        model.train()
        opt = build_optimizer(cfg, model)
        opt.enable_pipelined()
        np.random.seed(77)
        it = iter(D.build_detection_train_loader(cfg, recs, device=device))
        window = [next(it) for _ in range(2 * group)]
        assert all(len(x["proposals"]) == 30 and tuple(x["image"].shape) == (3, 64, 85) for b in window for x in b)
        assert all(x["image"].is_cuda == (device is not None) for b in window for x in b)
        stepper = GraphedTrainStep(model, opt, window[0], split_tail=True, trunk_pairs=True, eager_fc6=True, ring=True)
        out = []
        for _ in range(steps):
            losses = stepper.step(*window)
            out.append(torch.stack([losses[k].detach().clone().reshape(()) for k in sorted(losses)]))  # (no sync: a device copy)
            window = window[1:] + [next(it)]
        assert stepper._ring_on
        torch.cuda.synchronize()
        results.append(torch.stack(out).cpu())
        stepper.release()
        del stepper, model, opt
    assert torch.isfinite(results[0]).all()
    assert len({tuple(r.tolist()) for r in results[0]}) > steps // 2  # the batches really change the losses from step to step
    assert torch.equal(results[0], results[1])


def test_device_train_loader():
    """two passes over six records of two aspect ratios: CUDA fp32 images of their proposals' size, grouped as the host loader groups"""
    ocfg = G.MODEL_CASES["model_r50c4_tiny"]
    cfg = G.drn_cfg(ocfg, "cuda")
    cfg.merge_from_list(["INPUT.MIN_SIZE_TRAIN", "(48, 64)", "INPUT.CROP.ENABLED", "True", "SOLVER.IMS_PER_BATCH", "2",
                         "DATALOADER.NUM_WORKERS", "0", "DATASETS.PRECOMPUTED_PROPOSAL_TOPK_TRAIN", "30"])
    recs = _records(6, [(48, 64), (64, 48)], 40, 9, ocfg.num_classes)
    seen = []
    for device in (None, "cuda"):
        np.random.seed(13)
        it = iter(D.build_detection_train_loader(cfg, recs, device=device))
        batches = [next(it) for _ in range(6)]  # two passes: 12 images, 6 of either ratio, fill six batches of 2
        seen.append(batches)
        for b in batches:
            assert len(b) == 2 and len({x["width"] > x["height"] for x in b}) == 1
    assert len(seen[0]) == len(seen[1]) == 6
    for hb, db in zip(*seen):
        assert [x["image_id"] for x in hb] == [x["image_id"] for x in db]
        for hx, dx in zip(hb, db):
            im = dx["image"]
            assert im.is_cuda and im.dtype == torch.float32
            assert tuple(im.shape[1:]) == tuple(dx["proposals"].image_size) == tuple(hx["image"].shape[1:])
            assert "aug" not in dx and "image_src" not in dx
            assert torch.equal(dx["proposals"].proposal_boxes.tensor, hx["proposals"].proposal_boxes.tensor)
    assert len({x["image_id"] for b in seen[1] for x in b}) >= 5
