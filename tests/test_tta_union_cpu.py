"""GeneralizedRCNNWithTTAUNION, the parts that need no GPU: the names a driver ported from the reference imports, the C ABI of
the two new entries, the host mapper against the reference's golden, the host-side limits of ops.detect_union_batch, and the
numpy restatement of the merge (tests/tta_union_util.py) against the merged detections the reference itself produced - which
pins the helper the GPU tests compare the kernels with."""
import ctypes
import fnmatch
import importlib
import logging
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import golden_util as G
import tta_union_util as U
from __graft_entry__ import build, load_package

load_package()
from drn_wsod_pytorch_amd import ops  # noqa: E402
from drn_wsod_pytorch_amd._cabi import DrnError  # noqa: E402
from drn_wsod_pytorch_amd.structures import Boxes, Instances  # noqa: E402

O = G.O


def test_train_net_import_line_resolves():
    """projects/WSL/tools/train_net.py:46 as written, plus the mapper"""
    A = importlib.import_module("drn_wsod_pytorch_amd.aliases")
    A.install()
    try:
        from wsl.modeling import GeneralizedRCNNWithTTAAVG, GeneralizedRCNNWithTTAUNION  # noqa: F401
        from wsl.modeling import DatasetMapperTTAUNION
        import drn_wsod_pytorch_amd.modeling as M

        assert GeneralizedRCNNWithTTAUNION is M.GeneralizedRCNNWithTTAUNION and DatasetMapperTTAUNION is M.DatasetMapperTTAUNION
        assert GeneralizedRCNNWithTTAAVG is M.GeneralizedRCNNWithTTAAVG
    finally:
        A.uninstall()


def test_union_entries_declared_exported_and_bound():
    pkg = build()
    C = pkg._cabi
    hdr = open(os.path.join(G.ROOT, "include", "drn_wsod.h")).read()
    out = subprocess.check_output(["nm", "-D", "--defined-only", C.LIB_PATH], text=True)
    defined = {l.split()[-1] for l in out.splitlines() if l.strip()}
    emap = open(os.path.join(G.ROOT, "drn-wsod-pytorch_amd", "csrc", "exports.map")).read()
    globs = re.search(r"global:\s*([^;]*);", emap).group(1).split()
    lib = ctypes.CDLL(C.LIB_PATH)
    m = re.search(r"\bint\s+drn_detect_union_batch\s*\(([^;]*)\);", hdr)
    assert m, "include/drn_wsod.h does not declare drn_detect_union_batch"
    args = [" ".join(a.split()) for a in m.group(1).replace("\n", " ").split(",")]
    assert len(args) == 23 and args[-1] == "void* stream"
    assert [a.split()[-1].lstrip("*") for a in args] == [
        "blk_boxes", "blk_scores", "blk_classes", "blk_count", "n_blocks", "blk_topk", "img_off_host", "n_images", "tfm_host",
        "geom_host", "K", "score_thresh", "nms_thresh", "topk", "workspace", "workspace_bytes", "total_cap", "out_boxes",
        "out_scores", "out_classes", "out_rows", "out_count", "stream"]
    sig = C._SIGS["drn_detect_union_batch"]
    assert len(sig) == len(args)
    for ch, a in zip(sig, args):
        want = "p" if "*" in a else "f" if a.startswith("float") else "l" if a.startswith("long") else "i"
        assert ch == want, (a, ch)
    m = re.search(r"\blong\s+drn_detect_union_workspace_bytes\s*\(([^;]*)\);", hdr)
    assert m and [" ".join(a.split()) for a in m.group(1).split(",")] == ["int total_cap", "int n_images"]
    for name in ("drn_detect_union_batch", "drn_detect_union_workspace_bytes"):
        assert name in defined and hasattr(lib, name) and name in C.exported_symbols()
        assert any(fnmatch.fnmatchcase(name, g) for g in globs), "exports.map does not list %s" % name
    assert int(re.search(r"#define\s+DRN_DETECT_UNION_MAX_BLOCKS\s+(\d+)", hdr).group(1)) == ops.DETECT_UNION_MAX_BLOCKS == 256
    # the merge needs the batched tail's scratch and a little of its own
    assert C.lib().drn_detect_union_workspace_bytes(1600, 1) > C.lib().drn_detect_batch_workspace_bytes(1600, 1)
    # the existing entries keep their argument lists
    assert C._SIGS["drn_detect_topk_batch"] == "pppiiipi" + "ffi" + "pli" + "ppppp" + "p"


def _input(d):
    img = torch.from_numpy(d["image_u8"])
    H, W = img.shape[1:]
    prop = Instances((H, W))
    prop.proposal_boxes = Boxes(torch.from_numpy(d["proposal_boxes"]))
    prop.objectness_logits = torch.from_numpy(d["objectness_logits"])
    return {"image": img, "proposals": prop, "height": H, "width": W}


def test_host_mapper_matches_reference_golden(caplog):
    """the images bit for bit; the proposals are the input's own object, unchanged; the LOAD_PROPOSALS warning comes once"""
    import drn_wsod_pytorch_amd.modeling.tta as T

    d = G.load("tta_union_r50c4_tiny")
    cfg = G.drn_cfg(G.MODEL_CASES["model_r50c4_tiny"], "cpu")
    cfg.merge_from_list(U.tta_cfg_opts(d, 100))
    inp = _input(d)
    before = (d["proposal_boxes"].copy(), d["objectness_logits"].copy())
    mapper = T.DatasetMapperTTAUNION(cfg)
    T.DatasetMapperTTAUNION._warned = False
    with caplog.at_level(logging.WARNING):
        augs = mapper(inp)
        augs2 = mapper(inp)
    assert len([r for r in caplog.records if "DatasetMapperTTAUNION" in r.getMessage()]) == 1
    ref_avg = T.DatasetMapperTTAAVG(cfg)(inp)
    assert len(augs) == len(augs2) == int(d["n_aug"]) == 4
    H, W = inp["height"], inp["width"]
    for i, a in enumerate(augs):
        assert a["image"].dtype == torch.uint8 and np.array_equal(a["image"].numpy(), d["aug%d_image" % i]), i
        assert torch.equal(a["image"], ref_avg[i]["image"]) and a["tta"] == ref_avg[i]["tta"]
        assert a["proposals"] is inp["proposals"]
        assert np.array_equal(a["proposals"].proposal_boxes.tensor.numpy(), d["def_k100_aug%d_boxes" % i])
        assert np.array_equal(a["proposals"].objectness_logits.numpy(), d["def_k100_aug%d_obj" % i])
        assert tuple(a["proposals"].image_size) == tuple(int(v) for v in d["def_k100_aug%d_size" % i]) == (H, W)
        nh, nw = a["image"].shape[1:]
        assert a["tta"] == (W * 1.0 / nw, H * 1.0 / nh, float(nw) if i % 2 else -1.0)
        assert a["height"] == H and a["width"] == W
    assert np.array_equal(inp["proposals"].proposal_boxes.tensor.numpy(), before[0])
    assert np.array_equal(inp["proposals"].objectness_logits.numpy(), before[1])
    with pytest.raises(DrnError):  # an already resized input (pre_tfm) is refused as in the AVG mapper
        mapper(dict(inp, height=H * 2, width=W * 2))


def test_ops_limits_raise_without_a_library_call(monkeypatch):
    from drn_wsod_pytorch_amd import _cabi as C

    def no_lib(*a, **k):
        raise AssertionError("the library was touched")

    monkeypatch.setattr(C, "lib", no_lib)
    monkeypatch.setattr(C, "call", no_lib)

    def run(B=2, T=5, n_img=1, topk=10, off=None, **kw):
        z = lambda *s, dt=torch.float32: torch.zeros(s, dtype=dt)
        off = [0] + [B] * n_img if off is None else off
        return ops.detect_union_batch(kw.get("boxes", z(B, T, 4)), z(B, T), z(B, T, dt=torch.int32), z(B, dt=torch.int32), off,
                                      kw.get("tfms", [(1.0, 1.0, -1.0)] * B), [(8, 8)] * n_img, num_classes=3, nms_thresh=0.3,
                                      topk=topk)

    for bad in (dict(n_img=17), dict(B=257), dict(T=1025), dict(topk=1025), dict(topk=0), dict(off=[0, 1]), dict(off=[1, 2]),
                dict(off=[0, 3, 2], n_img=2), dict(tfms=[(1.0, 1.0, -1.0)]), dict(boxes=torch.zeros((2, 4, 4)))):
        with pytest.raises(DrnError):
            run(**bad)
    with pytest.raises(AssertionError, match="the library was touched"):
        run()  # within the limits the call goes through to the library


@pytest.mark.parametrize("tag,topk", U.CASES)
def test_numpy_merge_reproduces_reference_golden(tag, topk):
    """the recorded per-pass detections -> union rows -> merged detections, exactly as the reference produced both"""
    d = G.load("tta_union_r50c4_tiny")
    pre = "%s_k%d_" % (tag, topk)
    bb, bs, bc, cnt, tfms = U.golden_blocks(d, tag, topk)
    ub, us, uc = U.union_rows(bb, bs, bc, cnt, tfms)
    assert np.array_equal(ub, d[pre + "union_boxes"]) and np.array_equal(us, d[pre + "union_scores"])
    assert np.array_equal(uc, d[pre + "union_classes"])
    # the two-step corner transform of the helper is the oracle's TransformList restatement
    for i, (sx, sy, fw) in enumerate(tfms):
        steps = ([("hflip", int(fw))] if fw >= 0 else []) + [("scale", sx, sy)]
        assert np.array_equal(U.inverse_box(bb[i, : cnt[i]], sx, sy, fw), O.tta_apply_box(bb[i, : cnt[i]], steps))
    H, W = d["image_u8"].shape[1:]
    rb, rs, rc, rr = U.merge(ub, us, uc, (H, W), int(d["num_classes"]), float(d["nms_thresh"]), topk)
    assert np.array_equal(rc, d[pre + "det_classes"]) and np.array_equal(rs, d[pre + "det_scores"])
    assert np.array_equal(rb, d[pre + "det_boxes"])
    assert np.array_equal(rr, d[pre + "det_rows"]) and np.array_equal(us[rr], rs) and len(rs) > 0
    if tag == "avg":
        assert float(d[pre + "nms_pair_score_gap"]) > 1e-5  # no pair whose order decides a suppression sits closer than that
    if tag == "avg":
        assert float(d[pre + "iou_margin"]) > 1e-3 and float(d[pre + "score_gap"]) > 1e-5
    if (tag, topk) == ("avg", 100):
        assert len(rs) < min(len(us), topk)  # the NMS suppresses across augmentations
    if topk == 12:
        assert len(rs) == 12 < len(us)  # the top-k cuts
    if (tag, topk) == ("def", 100):
        assert len(us) - len(np.unique(us)) > 0  # exact score ties: their order is the union order
