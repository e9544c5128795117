"""PCL on image batches, the parts that need no GPU: the C ABI of the two batch entries (header, exports, _cabi), the batch
definition restated in tests/pcl_batch_util.py on the oracle's per-image functions, and the opt-in of PCLROIHeads."""
import ctypes
import fnmatch
import os
import re
import subprocess

import numpy as np
import pytest

import golden_util as G
import pcl_batch_util as U
from __graft_entry__ import build, load_package

load_package()
from drn_wsod_pytorch_amd._cabi import DrnError  # noqa: E402
from drn_wsod_pytorch_amd.modeling import build_model  # noqa: E402

ADJ_ARGS = ["const float* boxes", "const int* img_off", "int n_img", "int M", "int max_rows", "float iou_thr",
            "uint32_t* adj", "void* stream"]
REFINE_ARGS = ["const float* logits", "int ld", "const int* cols", "int n_branch", "int K", "const float* wsddn_scores",
               "int ld_ws", "const float* boxes", "const uint32_t* adj", "const float* onehot", "const int* img_off",
               "int n_img", "int M", "int max_rows", "float* probs", "int* labels", "float* cls_w", "int* assign",
               "int* pc_labels", "float* pc_probs", "int* pc_count", "float* img_w", "int* pc_rows", "float* pc_scores",
               "int* n_pc", "int pmax", "float* loss_img", "float* losses", "float* dlogits", "void* stream"]


def _decl(hdr, name):
    m = re.search(r"\bint\s+%s\s*\(([^;]*)\);" % name, hdr)
    assert m, "include/drn_wsod.h does not declare %s" % name
    return [" ".join(a.split()) for a in m.group(1).replace("\n", " ").split(",")]


def test_header_declares_the_batch_entries():
    hdr = open(os.path.join(G.ROOT, "include", "drn_wsod.h")).read()
    assert _decl(hdr, "drn_pcl_adjacency_batch") == ADJ_ARGS
    assert _decl(hdr, "drn_pcl_refine_batch") == REFINE_ARGS
    assert re.search(r"#define\s+DRN_PCL_MAX_IMAGES\s+(\d+)", hdr) and int(re.search(
        r"#define\s+DRN_PCL_MAX_IMAGES\s+(\d+)", hdr).group(1)) >= 8
    # the single-image entries keep their argument lists
    assert len(_decl(hdr, "drn_pcl_adjacency")) == 5 and len(_decl(hdr, "drn_pcl_refine")) == 26


def test_batch_entries_exported_and_bound():
    pkg = build()
    C = pkg._cabi
    out = subprocess.check_output(["nm", "-D", "--defined-only", C.LIB_PATH], text=True)
    defined = {l.split()[-1] for l in out.splitlines() if l.strip()}
    emap = open(os.path.join(G.ROOT, "drn-wsod-pytorch_amd", "csrc", "exports.map")).read()
    globs = re.search(r"global:\s*([^;]*);", emap).group(1).split()
    lib = ctypes.CDLL(C.LIB_PATH)
    for name, args in (("drn_pcl_adjacency_batch", ADJ_ARGS), ("drn_pcl_refine_batch", REFINE_ARGS)):
        assert name in defined and hasattr(lib, name) and name in C.exported_symbols()
        assert any(fnmatch.fnmatchcase(name, g) for g in globs), "exports.map does not list %s" % name
        sig = C._SIGS[name]
        assert len(sig) == len(args)
        for ch, a in zip(sig, args):
            assert ch == ("p" if "*" in a else "f" if a.startswith("float") else "i"), (name, a, ch)
    assert C._SIGS["drn_pcl_adjacency"] == "pifpp" and len(C._SIGS["drn_pcl_refine"]) == 26


def test_batch_oracle_satisfies_the_definition():
    """3 images (one without labels): per-image parts are the oracle's own single-image results, the batch loss is the fp64
    mean in ascending order rounded once, the gradient rows are the single-image rows times float32(1/3)"""
    from oracle import pcl_oracle as PO

    K, nb = 5, 2
    images = [U.make_image(R, K, nb, nl, 50 + i) for i, (R, nl) in enumerate(((40, 2), (23, 0), (57, 1)))]
    ref = U.batch_oracle(images)
    assert ref["loss_img"].shape == (3, nb) and ref["loss_img"].dtype == np.float32
    third = np.float32(1.0) / np.float32(3.0)
    for i, img in enumerate(images):
        prev = img["last"]
        for b in range(nb):
            with np.errstate(all="ignore"):
                loss, dl, probs, t = PO.pcl_refine_loss(img["logits"][b], img["boxes"], prev, img["im"])
            got = ref["per_image"][i][b]
            assert np.float32(loss) == ref["loss_img"][i, b] == got[0]
            assert np.array_equal(got[3]["labels"], t["labels"]) and np.array_equal(got[3]["gt_assignment"], t["gt_assignment"])
            assert got[3]["gt_assignment"].max(initial=-1) < len(t["pc_labels"])  # centre indices local to the image
            want = (dl.astype(np.float32) * third).astype(np.float32)
            assert ref["dlogits"][i][b].dtype == np.float32 and np.array_equal(ref["dlogits"][i][b], want)
            prev = probs
    assert ref["loss_img"][1].tolist() == [0.0, 0.0] and not np.any(ref["dlogits"][1][0])  # the image without labels
    for b in range(nb):
        l = ref["loss_img"][:, b].astype(np.float64)
        assert ref["loss"][b] == np.float32(((l[0] + l[1]) + l[2]) / 3.0)
    assert ref["loss"].dtype == np.float32
    # exact scaling for powers of two, and n = 1 changes nothing
    x = ref["per_image"][0][0][1]
    assert np.array_equal(U.scale_rows(x, 1), x) and np.array_equal(U.scale_rows(x, 4) * np.float32(4), x)
    assert U.batch_mean(ref["loss_img"][:1]).tolist() == ref["loss_img"][0].tolist()


def test_enable_image_batches_exists_and_defaults_to_off():
    cfg = G.drn_cfg(G.MODEL_CASES["model_pcl_r50c4_tiny"], "cpu")
    heads = build_model(cfg).roi_heads
    assert type(heads).__name__ == "PCLROIHeads"
    assert heads.image_batches is False and not getattr(heads._engine, "pcl_image_batches", False)
    assert not hasattr(cfg.WSL, "PCL_IMAGE_BATCHES")  # a method, not a config key
    assert heads.enable_image_batches(True) is heads and heads.image_batches is True
    heads.enable_image_batches(False)
    assert heads.image_batches is False


def test_ops_refuse_bad_batches_on_the_host():
    """the checks that need no device: image count, max_rows, and - with img_off on the host, where the sizes are known - an
    image above max_rows or an img_off that does not split the rows"""
    import torch
    from drn_wsod_pytorch_amd import ops

    boxes = torch.zeros((60, 4))
    off = lambda *o: torch.tensor(o, dtype=torch.int32)
    assert ops.PCL_MAX_IMAGES >= 8 and ops.PCL_MAX_ROWS == 4096
    for img_off, n, max_rows in ((off(0, 10, 60), 2, 40),            # R_1 = 50 > max_rows
                                 (off(0, 10, 50), 2, 50),            # does not end at M
                                 (off(0, 60, 60), 2, 60),            # an empty image
                                 (off(*range(0, 72, 4))[:18], 17, 60),   # 17 images
                                 (off(0, 10, 60), 2, 4097)):         # max_rows above the per-image limit
        with pytest.raises(DrnError):
            ops.pcl_adjacency_batch(boxes, img_off, n, max_rows, 0.4)
