"""Shared by tests/test_augment_cpu.py and tests/test_augment_gpu.py: the device mapper's arithmetic restated in plain numpy
(the specification of drn_augment_u8), and the record / config / seed of tests/golden/data_mapper.npz exactly as
tests/test_surface_cpu.py::test_data_path_matches_reference_golden builds them."""
import pickle

import numpy as np
import torch

import golden_util as G

GOLDEN_OVERRIDES = ["INPUT.MIN_SIZE_TRAIN", "(48, 64, 80)", "INPUT.MAX_SIZE_TRAIN", "120", "INPUT.MIN_SIZE_TEST", "64",
                    "INPUT.MAX_SIZE_TEST", "100", "INPUT.CROP.ENABLED", "True",
                    "DATASETS.PRECOMPUTED_PROPOSAL_TOPK_TRAIN", "30", "DATASETS.PRECOMPUTED_PROPOSAL_TOPK_TEST", "25"]


def pil_resize(img, new_h, new_w):
    """Pillow's BILINEAR resize of an HWC uint8 image, channel by channel (a 4-channel image must not go through Pillow's RGBA
    mode, which pre-multiplies alpha: the oracle's restatement of Resample.c, pinned against Pillow by tests/test_oracle_golden.py)"""
    from PIL import Image

    if img.shape[:2] == (new_h, new_w):
        return img
    if img.shape[2] == 3:
        return np.asarray(Image.fromarray(np.ascontiguousarray(img)).resize((new_w, new_h), Image.BILINEAR))
    if img.shape[2] == 1:
        return np.asarray(Image.fromarray(np.ascontiguousarray(img[:, :, 0])).resize((new_w, new_h), Image.BILINEAR))[:, :, None]
    return G.O.pil_bilinear_resize_u8(np.ascontiguousarray(img), new_h, new_w)


def restate(src, aug):
    """src uint8 [H, W, C] (numpy), aug = plan()'s dict -> uint8 [C, Ho, Wo]: crop, Pillow BILINEAR, flip, then
    B = u8(clip(f32(wb) * f32(R))) and u8(clip((1 - ws) * g + f64(f32(ws) * f32(B)))) with the grey value g summed in
    index order in float64: ((B0 * 0.299 + B1 * 0.587) + B2 * 0.114)"""
    x0, y0, cw, ch = aug["crop"]
    ho, wo = aug["out_hw"]
    r = pil_resize(src[y0: y0 + ch, x0: x0 + cw], ho, wo)
    if aug["flip"]:
        r = r[:, ::-1]
    if aug["wb"] is not None:
        r = np.clip(np.float32(aug["wb"]) * r.astype(np.float32), 0, 255).astype(np.uint8)
    if aug["ws"] is not None:
        assert r.shape[2] == 3
        ws = float(aug["ws"])
        b = r.astype(np.float64)
        g = ((b[:, :, 0] * 0.299 + b[:, :, 1] * 0.587) + b[:, :, 2] * 0.114)[:, :, None]
        t = (1 - ws) * g + (np.float32(ws) * r.astype(np.float32)).astype(np.float64)
        r = np.clip(t, 0, 255).astype(np.uint8)
    return np.ascontiguousarray(r.transpose(2, 0, 1))


def golden_record(tmp_path):
    """-> (golden arrays, cfg, [record with proposals loaded]) of data_mapper.npz"""
    from PIL import Image

    from __graft_entry__ import load_package

    load_package()
    from drn_wsod_pytorch_amd import data as D

    d = G.load("data_mapper")
    cfg = G.drn_cfg(G.MODEL_CASES["model_r50c4_tiny"], "cpu")
    cfg.merge_from_list(GOLDEN_OVERRIDES)
    rgb = d["rgb"]
    H, W = rgb.shape[:2]
    fn = str(tmp_path / "000123.png")
    Image.fromarray(rgb).save(fn)
    pf = str(tmp_path / "props.pkl")
    with open(pf, "wb") as f:
        pickle.dump({"indexes": [7, 123], "boxes": [np.zeros((3, 4), np.float32), d["boxes"]],
                     "scores": [np.zeros(3, np.float32), d["scores"]]}, f)
    annos = [{"bbox": [10.0, 8.0, 50.0, 40.0], "bbox_mode": 0, "category_id": 3},
             {"bbox": [30.5, 20.25, 80.0, 58.0], "bbox_mode": 0, "category_id": 1},
             {"bbox": [5.0, 5.0, 20.0, 20.0], "bbox_mode": 0, "category_id": 2, "iscrowd": 1}]
    rec = {"file_name": fn, "height": H, "width": W, "image_id": 123, "annotations": annos}
    return d, cfg, D.load_proposals_into_dataset([dict(rec)], pf)


def assert_boxes_equal_golden(out, d, k, is_train):
    assert np.array_equal(out["proposals"].proposal_boxes.tensor.numpy(), d[k + "prop_boxes"]), k
    assert np.array_equal(out["proposals"].objectness_logits.numpy(), d[k + "prop_logits"]), k
    if is_train:
        assert np.array_equal(out["instances"].gt_boxes.tensor.numpy(), d[k + "gt_boxes"]), k
        assert np.array_equal(out["instances"].gt_classes.numpy(), d[k + "gt_classes"]), k


def assert_items_equal(a, b):
    """two mapper outputs (planned or finished), field by field"""
    assert set(a) == set(b), (sorted(a), sorted(b))
    for key, va in a.items():
        vb = b[key]
        if torch.is_tensor(va):
            assert va.dtype == vb.dtype and torch.equal(va.cpu(), vb.cpu()), key
        elif key in ("proposals", "instances"):
            assert va.image_size == vb.image_size, key
            fa, fb = va.get_fields(), vb.get_fields()
            assert set(fa) == set(fb), key
            for name in fa:
                ta = fa[name].tensor if hasattr(fa[name], "tensor") else fa[name]
                tb = fb[name].tensor if hasattr(fb[name], "tensor") else fb[name]
                assert torch.equal(ta, tb), (key, name)
        else:
            assert va == vb, key
