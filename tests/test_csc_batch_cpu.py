"""CSC on image batches, the parts that need no GPU: the opt-in of CSCROIHeads, the C ABI of the four batch entries (header,
exports, _cabi), the slot schedule as a pure function, the schedule's one-upload layout, and the limits refused on the host."""
import ctypes
import fnmatch
import os
import re
import subprocess

import pytest
import torch

import golden_util as G
from __graft_entry__ import build, load_package

load_package()
from drn_wsod_pytorch_amd import ops  # noqa: E402
from drn_wsod_pytorch_amd._cabi import DrnError  # noqa: E402
from drn_wsod_pytorch_amd.modeling import build_model  # noqa: E402
from drn_wsod_pytorch_amd.modeling.roi_heads import csc_slot_schedule  # noqa: E402

ENTRIES = {"drn_csc_seed_batch": 14, "drn_csc_cpg_batch": 14, "drn_csc_weights_batch": 21, "drn_csc_loss_batch": 18}


def _decl(hdr, name):
    m = re.search(r"\bint\s+%s\s*\(([^;]*)\);" % name, hdr)
    assert m, "include/drn_wsod.h does not declare %s" % name
    return [" ".join(a.split()) for a in m.group(1).replace("\n", " ").split(",")]


def test_enable_image_batches_exists_and_defaults_to_off():
    cfg = G.drn_cfg(G.csc_case(), "cpu")
    heads = build_model(cfg).roi_heads
    assert type(heads).__name__ == "CSCROIHeads"
    assert heads.image_batches is False
    assert not hasattr(cfg.WSL, "CSC_IMAGE_BATCHES")  # a method, not a config key
    with pytest.raises(AttributeError):
        heads.image_batches = True  # read-only
    assert heads.enable_image_batches(True) is heads and heads.image_batches is True
    assert heads.enable_image_batches(False) is heads and heads.image_batches is False
    assert heads.enable_image_batches() is heads and heads.image_batches is True


def test_batch_entries_declared_exported_and_bound():
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
        assert name in defined and hasattr(lib, name) and name in C.exported_symbols()
        assert any(fnmatch.fnmatchcase(name, g) for g in globs), "exports.map does not list %s" % name
        sig = C._SIGS[name]
        assert len(sig) == len(args)
        for ch, a in zip(sig, args):
            want = "p" if "*" in a else "f" if a.startswith("float") else "l" if a.startswith("long") else "i"
            assert ch == want, (name, a, ch)
        assert hasattr(ops, name[len("drn_"):])
    assert int(re.search(r"#define\s+DRN_CSC_MAX_IMAGES\s+(\d+)", hdr).group(1)) == ops.CSC_MAX_IMAGES == 16
    assert ops.CSC_MAX_K == 128
    assert "CSC on image batches" in hdr
    # the single-image entries keep their argument lists
    assert C._SIGS["drn_csc_cpg"] == "piiiiippp" and len(_decl(hdr, "drn_csc_weights")) == 14
    assert len(_decl(hdr, "drn_csc_loss")) == 17
    mk = open(os.path.join(G.ROOT, "drn-wsod-pytorch_amd", "csrc", "Makefile")).read()
    assert "build/csc.o" in mk and "csc" not in mk.split("CONTRACT_OBJS =")[1].split("\n")[0]  # -ffp-contract=off


def test_slot_schedule():
    """labelled sets [[1,3],[0],[2,3,5]], tau = 0.5: class 3 of image 0 is below tau, image 1 has no active class, and the
    images have 1, 0 and 3 active classes"""
    K = 6
    s = [[0.0] * K for _ in range(3)]
    s[0][1], s[0][3] = 0.9, 0.49
    s[0][0] = 0.99             # not labelled: never active
    s[1][0] = 0.1
    s[2][2], s[2][3], s[2][5] = 0.5, 0.7, 1.0   # exactly tau counts (>=)
    sch = csc_slot_schedule([[1, 3], [0], [2, 3, 5]], s, 0.5)
    assert sch["active"] == [[1], [], [2, 3, 5]]
    assert sch["slots"] == [[1, -1, 2], [-1, -1, 3], [-1, -1, 5]]
    assert sch["pairs"] == [(0, 1), (0, 3), (1, 0), (2, 2), (2, 3), (2, 5)]
    # tensors / unsorted / repeated labels (gt_classes_img_int holds unique sorted ints; the function does not rely on it)
    sch2 = csc_slot_schedule([torch.tensor([3, 1, 3]).tolist(), [0], [5, 2, 3]], s, 0.5)
    assert sch2 == sch
    # nothing active: no slot, every labelled class still a pair
    none = csc_slot_schedule([[1, 3], [0]], s[:2], 2.0)
    assert none["slots"] == [] and none["active"] == [[], []] and none["pairs"] == [(0, 1), (0, 3), (1, 0)]
    # tau = 0: every labelled class is active; S = the largest label set, not the sum
    allc = csc_slot_schedule([[1, 3], [0], [2, 3, 5]], s, 0.0)
    assert len(allc["slots"]) == 3 and sum(c >= 0 for row in allc["slots"] for c in row) == 6
    assert csc_slot_schedule([[4]], [[0.0] * 4 + [1.0]], 0.7) == dict(active=[[4]], slots=[[4]], pairs=[(0, 4)])


def test_plan_is_one_upload_with_the_documented_layout():
    sizes = [(4, 7), (3, 5), (4, 6)]
    sch = csc_slot_schedule([[1, 3], [0], [2, 3, 5]], [[1.0] * 6] * 3, 0.5)
    plan = ops.CscBatchPlan(sizes, 6, sch["slots"], sch["pairs"], "cpu")
    n, S, P = 3, 3, 6
    assert plan.words.dtype == torch.int64 and plan.words.numel() == 2 * n + n + S * n + 2 * P + P
    assert plan.words[:6].tolist() == [4, 7, 3, 5, 4, 6]
    assert plan.d_map_off.tolist() == [0, 6 * 28, 6 * 28 + 6 * 15] and plan.map_floats == 6 * (28 + 15 + 24)
    assert [t.tolist() for t in plan.d_slots] == [[1, 0, 2], [3, -1, 3], [-1, -1, 5]]
    assert plan.d_pairs.tolist() == [0, 1, 0, 3, 1, 0, 2, 2, 2, 3, 2, 5]
    assert plan.d_tab_off.tolist() == [0, 28, 56, 71, 95, 119] and plan.table_floats == 143
    assert (plan.Hmax, plan.Wmax, plan.max_px) == (4, 7, 28)
    for t in [plan.d_hw, plan.d_map_off, plan.d_pairs, plan.d_tab_off] + plan.d_slots:  # views of the ONE tensor
        assert t.untyped_storage().data_ptr() == plan.words.untyped_storage().data_ptr()
    flat, maps = plan.new_maps("cpu")
    assert [tuple(m.shape) for m in maps] == [(6, 4, 7), (6, 3, 5), (6, 4, 6)] and not flat.any()
    with pytest.raises(DrnError):
        ops.CscBatchPlan(sizes, 6, [[1, 0]], sch["pairs"], "cpu")        # a slot row of the wrong length
    with pytest.raises(DrnError):
        ops.CscBatchPlan(sizes, 6, sch["slots"], [(0, 1), (0, 1)], "cpu")  # a repeated pair
    with pytest.raises(DrnError):
        ops.CscBatchPlan(sizes, 6, sch["slots"], [(3, 1)], "cpu")          # an image that is not there


def test_limits_are_refused_on_the_host():
    """more than 16 images, K > 128, an image of 2^24 pixels: DrnError before any pointer is taken (CPU tensors never reach
    the library)"""
    z = torch.zeros
    off17 = torch.arange(18, dtype=torch.int32)
    with pytest.raises(DrnError, match="17 images"):
        ops.csc_batch_limits(17, 20)
    with pytest.raises(DrnError, match="K = 129"):
        ops.csc_batch_limits(2, 129)
    with pytest.raises(DrnError, match="pixels"):
        ops.csc_batch_limits(1, 20, [(4096, 4096)])
    ops.csc_batch_limits(16, 128, [(4096, 4095)])
    with pytest.raises(DrnError):
        ops.csc_seed_batch(z(17, 40), 0, 20, 20, z(17, 20), z(17, 20), off17, 17, z(17, dtype=torch.int64), z(17, 40))
    with pytest.raises(DrnError):
        ops.csc_seed_batch(z(2, 258), 0, 129, 129, z(2, 129), z(2, 129), off17[:3], 2, z(2, dtype=torch.int64), z(2, 258))
    with pytest.raises(DrnError):
        ops.csc_loss_batch(z(17, 40), 0, 20, 20, z(17, 20), z(17, 20), None, z(17, 20), off17, 17, False)
    with pytest.raises(DrnError):
        ops.csc_loss_batch(z(2, 258), 0, 129, 129, z(2, 129), z(2, 129), None, z(2, 129), off17[:3], 2, False)
    with pytest.raises(DrnError):
        ops.CscBatchPlan([(8, 8)] * 17, 20, [], [], "cpu")
    with pytest.raises(DrnError):
        ops.CscBatchPlan([(8, 8)] * 2, 129, [], [], "cpu")
    with pytest.raises(DrnError):
        ops.CscBatchPlan([(8, 8), (4096, 4096)], 20, [], [], "cpu")
    # the library's own host checks answer the same before any launch (null pointers are never dereferenced on this path)
    lib = build()._cabi.lib()
    assert lib.drn_csc_seed_batch(None, 40, 0, 20, 20, None, None, None, 17, 17, None, None, 40, None) == -3
    assert lib.drn_csc_loss_batch(None, 258, 0, 129, 129, None, None, None, None, None, 2, 2, 0, None, None, None, 258, None) == -3
