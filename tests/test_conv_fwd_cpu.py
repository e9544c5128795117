"""CPU checks of what test_conv_fwd_gpu.py holds the forward conv kernels to (conv_fwd_util.py):
  1. the plan table: every case plans to the kernel it claims on a 256-CU device under its knobs (host-only ops.conv2d_plan), the
     knobs are restored afterwards, every kind of ops.CONV_KIND_* except FP8_K16 has a bf16 case and the five generic ones an fp32
     case, the mixed-storage cases stay off the bf16-only kernels, and TILED_128X64 / TILED_128 give way to TILED_64 below their
     threshold;
  2. grid exactness: for every case max sum|x||w| * 2^5 < 2^24, an fp32 F.conv2d with permuted input channels equals the float64
     one bit for bit, the fp8 case stays inside +-448, and the grid really produces ties at the bf16 store;
  3. teeth: a plain torch emulation of the device arithmetic passes both checks, and each planted fault - a truncating bf16 store,
     a bf16-rounded BN scale, a bf16 rounding in front of the shortcut add, one missing product at the last pixel, eight missing
     channels of one tap on the last row - fails at least one of them wherever it applies.
No GPU is needed; the printed ratios (pytest -s) are the emulation's, not a device's."""
import importlib

import pytest
import torch
import torch.nn.functional as F

import conv_fwd_util as V
from __graft_entry__ import build


@pytest.fixture(scope="module")
def ops():
    build()
    return importlib.import_module("drn_wsod_pytorch_amd.ops")


# ---- 1. the plan table -------------------------------------------------------------------------------------------------------------
def test_case_table_covers_every_kind(ops):
    kinds = {getattr(ops, n): n[len("CONV_KIND_"):] for n in dir(ops) if n.startswith("CONV_KIND_") and n != "CONV_KIND_FP8_K16"}
    assert kinds == V.KIND_NAMES
    plain = [c for c in V.CASES if c.out_dtype == c.dtype and c.res_dtype == c.dtype]
    assert {c.kind for c in plain if c.dtype == V.BF16} == set(V.KIND_NAMES.values())
    assert {c.kind for c in plain if c.dtype == V.F32} == {"K2", "KS", "TILED_64", "TILED_128X64", "TILED_128"}
    assert all(set(c.forms) == set(V.FORMS) for c in plain)
    assert len({V.case_id(c) for c in V.CASES}) == len(V.CASES)
    for c in V.CASES:  # the smallest shapes that still have the edges, no workload-size map: every reference conv stays under 0.4 G multiply-adds
        n, h, w_, cin, cout, k, stride, pad, dil = c.shape
        ho, wo = V.out_hw(h, w_, k, stride, pad, dil)
        assert cin * k * k <= 4608 and n * ho * wo * cout * cin * k * k < 4e8, V.case_id(c)


@pytest.mark.parametrize("case", V.CASES, ids=V.case_id)
def test_case_plans_to_its_kind(ops, case):
    defaults = [V.plan_name(ops, case, f) for f in case.forms]
    with ops.tuned(V.knob_dict(ops, case)):
        for form in case.forms:
            assert V.plan_name(ops, case, form) == case.kind, (V.case_id(case), form)
    assert [V.plan_name(ops, case, f) for f in case.forms] == defaults  # the knobs are back
    if case.out_dtype != case.dtype or case.res_dtype != case.dtype:
        assert case.kind not in V.BF16_ONLY_KINDS


@pytest.mark.parametrize("dtype", [V.F32, V.BF16], ids=V.dname)
def test_tiled_128_kinds_give_way_below_their_threshold(ops, dtype):
    """The tiled kernels are chosen on the batch's count of 128-row x 128-column tiles: below 128 of them TILED_64, from 128 on
    TILED_128X64 (Cout <= 64) or TILED_128.  The TILED_128X64 case sits on the threshold itself (128 x 129 pixels, one column tile:
    one step smaller, 127 x 128, is TILED_64); the TILED_128 case is sized for its ragged tiles (32 x 5), so its threshold is
    looked up here on the same layer: 25 row tiles x 5 column tiles = 125 plan to TILED_64, one more pixel column makes it 26 x 5."""
    by_kind = {c.kind: c for c in V.CASES if c.dtype == dtype and c.out_dtype == dtype and c.res_dtype == dtype}
    c = by_kind["TILED_128X64"]
    n, h, w_ = c.shape[:3]
    for form in c.forms:
        assert V.plan_name(ops, c, form) == "TILED_128X64"
        assert V.plan_name(ops, c, form, shape=(n, h - 1, w_ - 1) + c.shape[3:]) == "TILED_64"
    c = by_kind["TILED_128"]
    for form in c.forms:
        assert V.plan_name(ops, c, form) == "TILED_128"
        assert V.plan_name(ops, c, form, shape=(1, 50, 64) + c.shape[3:]) == "TILED_64"     # 3200 pixels: 25 row tiles
        assert V.plan_name(ops, c, form, shape=(1, 50, 65) + c.shape[3:]) == "TILED_128"    # 3250 pixels: 26 row tiles


# ---- 2. the grid is exact ------------------------------------------------------------------------------------------------------------
GRID_CASES = {(c.shape, c.dtype, k): c for c in V.CASES for k in c.inputs if k != "general"}


@pytest.mark.parametrize("key", sorted(GRID_CASES, key=str), ids=lambda k: "%s-%s-%s" % (k[0], V.dname(k[1]), k[2]))
def test_grid_accumulates_exactly_in_fp32(key):
    shape, dtype, kind = key
    case = GRID_CASES[key]
    n, h, w_, cin, cout, k, stride, pad, dil = shape
    p = V.inputs(shape, dtype, kind)
    x, wt = p["x"], p["w"]
    assert torch.equal(x, x.to(V.BF16).float()) and torch.equal(wt, wt.to(V.BF16).float())  # on the grid in either dtype
    assert torch.equal(x * 4, (x * 4).round()) and x.abs().max() <= 2 and torch.equal(wt * 8, (wt * 8).round()) and wt.abs().max() <= 1
    for t in (p["bias"], p["res"]):
        assert torch.equal(t * 4, (t * 4).round()) and t.abs().max() <= 4
    mag = F.conv2d(x.double().abs(), wt.double().abs(), None, stride, pad, dil)
    assert float(mag.max()) * 2 ** 5 < 2 ** 24 and cin * k * k <= 4608
    # whatever the order of the sum: input channels permuted, float32, against float64
    perm = torch.randperm(cin, generator=torch.Generator().manual_seed(3))
    y32 = F.conv2d(x[:, perm].contiguous(), wt[:, perm].contiguous(), None, stride, pad, dil)
    y64 = F.conv2d(x.double(), wt.double(), None, stride, pad, dil)
    assert torch.equal(y32.double(), y64)
    # ... and the epilogue: the float64 reference of every form is a float32 number
    for form in case.forms:
        ref, _ = V.reference(case, form, kind)
        assert torch.equal(ref.float().double(), ref), form
        if case.out_dtype == V.FP8:
            assert float(ref.abs().max()) <= V.FP8_MAX
            assert not V.stored(ref, V.FP8).float().isnan().any()


def test_grid_has_ties_at_the_bf16_store():
    """round-to-nearest-even is only pinned if some exact results lie half-way between two bf16 numbers, with both parities"""
    case = next(c for c in V.CASES if c.kind == "TILED_64" and c.tag == "A" and c.dtype == V.BF16 and c.out_dtype == V.BF16)
    ref, _ = V.reference(case, "bn_res", "grid")
    y = ref.float()
    bits = y.contiguous().view(torch.int32)
    tie = (bits & 0xFFFF) == 0x8000
    assert int(tie.sum()) >= 20
    up = V.stored(ref, V.BF16).float().abs() > y.abs()
    assert bool((tie & up).any()) and bool((tie & ~up).any())  # ties that go up and ties that go down


# ---- 3. teeth ------------------------------------------------------------------------------------------------------------------------
def _teeth_case(shape_tag, kind="TILED_64"):
    return next(c for c in V.CASES if c.kind == kind and c.tag == shape_tag and c.dtype == V.BF16 and c.out_dtype == V.BF16
                and c.res_dtype == V.BF16)


def _checks(case, form, kind, got):
    """(general check passes, grid check passes) - the second is None on general input"""
    ref, bound = V.reference(case, form, kind)
    if kind == "general":
        r = V.general_ratio(got.float(), ref, bound)
        print("RATIO emulation %s %s %s %.4f" % (V.case_id(case), form, kind, r))
        return r <= 1.0, None
    r = V.general_ratio(got.float(), ref, bound)
    return r <= 1.0, not V.grid_mismatches(got, ref, case.out_dtype)


TEETH = [("A", "bn_relu"), ("A", "bn_res_relu"), ("D", "bn_res")]


@pytest.mark.parametrize("shape_tag,form", TEETH)
def test_clean_emulation_passes_both_checks(shape_tag, form):
    case = _teeth_case(shape_tag)
    ok, _ = _checks(case, form, "general", V.emulate(case, form, "general"))
    assert ok
    ok, exact = _checks(case, form, "grid", V.emulate(case, form, "grid"))
    assert ok and exact


@pytest.mark.parametrize("fault", V.FAULTS)
@pytest.mark.parametrize("shape_tag,form", TEETH)
def test_planted_fault_fails_a_check(shape_tag, form, fault):
    case = _teeth_case(shape_tag)
    if fault == "double_round" and form not in V.SHORTCUT_FORMS:
        # without a shortcut the early rounding IS the store: nothing is planted, and nothing may be seen
        for kind in ("general", "grid"):
            assert V.same_bits(V.emulate(case, form, kind, fault), V.emulate(case, form, kind))
        return
    ok_general, _ = _checks(case, form, "general", V.emulate(case, form, "general", fault))
    if fault == "bf16_scale":  # the grid's scales are bf16 numbers: applies on general input only
        assert not ok_general
        return
    ok_bound, exact = _checks(case, form, "grid", V.emulate(case, form, "grid", fault))
    print("fault %s on %s %s: general %s, grid bound %s, grid bits %s" % (fault, shape_tag, form, ok_general, ok_bound, exact))
    assert not ok_general or not exact
    if fault in ("trunc_store", "double_round", "missing_tap_channels"):
        assert not exact  # the bit-exact check alone sees these


def test_mixed_storage_emulation_passes():
    """the mixed-storage rows of the table (fp32 output, fp32 shortcut x 0.5, fp8 output) through the same two checks"""
    for case in V.CASES:
        if case.kind != "TILED_64" or (case.out_dtype == case.dtype and case.res_dtype == case.dtype):
            continue
        for form in case.forms:
            for kind in case.inputs:
                got = V.emulate(case, form, kind)
                ref, bound = V.reference(case, form, kind)
                if kind == "general":
                    assert V.general_ratio(got.float(), ref, bound) <= 1.0, (V.case_id(case), form)
                else:
                    assert not V.grid_mismatches(got, ref, case.out_dtype), (V.case_id(case), form)
