"""CPU tests of the tuning knobs (drn_tune needs no device, the two profile dumps - knob 28, knob 31 value 12 - apart):
ops.TUNE_* against the header, drn_tune's per-knob contract as a table of calls, and ops.tuned's save / restore."""
import ctypes
import importlib
import os
import re

import pytest

import golden_util as G
from __graft_entry__ import build


@pytest.fixture(scope="module")
def pkg():
    return build()


@pytest.fixture(scope="module")
def ops(pkg):
    return importlib.import_module("drn_wsod_pytorch_amd.ops")


def header_knobs():
    hdr = open(os.path.join(G.ROOT, "include", "drn_wsod.h")).read()
    return {name: int(val) for name, val in re.findall(r"^#define DRN_(TUNE_[A-Z0-9_]+)\s+(-?\d+)\b", hdr, re.M)}


def test_ops_knob_ids_equal_header(ops):
    hdr = header_knobs()
    assert len(hdr) == 29 and len(set(hdr.values())) == 29
    mine = {n: v for n, v in vars(ops).items() if n.startswith("TUNE_") and isinstance(v, int)}
    assert mine == hdr, set(mine.items()) ^ set(hdr.items())
    ids = [int(v) for v in re.findall(r"^#define DRN_TUNE_[A-Z0-9_]+\s+(\d+)", open(os.path.join(G.ROOT, "include", "drn_wsod.h")).read(), re.M)]
    assert ids == sorted(ids), "the header lists the knobs by ascending id"


# knob -> (default, [(value, what drn_tune returns = the setting BEFORE this call), ...]).  Every list starts at the default,
# ends with the call that restores it, and holds: an accepted non-default value read back by the next call, the values the
# knob rejects (the next call still returns the old setting), and the knob's quirks.  Recorded from the library as it was
# before the knobs moved into one table; the same table has to pass against any later build.
CONTRACT = {
    1: (1, [(0, 1), (7, 0), (0, 1), (-2, 0), (1, 1)]),                      # truthy
    2: (512, [(1024, 512), (7, 1024), (65536, 1024), (0, 1024), (8, 1024), (65535, 8), (512, 65535)]),  # 8..65535
    3: (0, [(8, 0), (65, 8), (-1, 8), (64, 8), (0, 64)]),                   # 0..64
    4: (512, [(1024, 512), (1, 1024), (300, 512), (2, 512), (0, 512), (256, 0), (512, 256)]),  # 1 -> 512; else 0 / 256 / 512 / 1024
    5: (1, [(0, 1), (7, 0), (0, 1), (-2, 0), (1, 1)]),
    6: (1, [(0, 1), (7, 0), (0, 1), (-2, 0), (1, 1)]),
    7: (0, [(40, 0), (-1, 40), (0, 40)]),                                   # >= 0
    8: (-1, [(0, -1), (-7, 0), (123456, -7), (-1, 123456)]),                # anything
    # returns the pixel threshold while on, 0 while off; a value > 1 also sets the threshold (1 turns on and keeps it)
    9: (32768, [(0, 32768), (1, 0), (5000, 32768), (1, 5000), (0, 5000), (-3, 0), (32768, 5000)]),
    10: (1, [(8, 1), (3, 8), (0, 8), (128, 8), (-4, 8), (64, 8), (1, 64)]),  # powers of two 1..64
    11: (1, [(0, 1), (7, 0), (0, 1), (-2, 0), (1, 1)]),
    12: (1, [(0, 1), (-3, 0), (2, 0), (1, 2)]),                             # negatives -> 0
    13: (1, [(0, 1), (7, 0), (0, 1), (-2, 0), (1, 1)]),
    14: (0, [(9, 0), (0, 1), (-1, 0), (0, 1)]),                             # truthy, default off
    15: (154, [(76, 154), (59, 76), (155, 76), (60, 76), (154, 60)]),       # 60..154
    18: (0, [(64, 0), (60, 64), (-8, 64), (4104, 64), (4096, 64), (0, 4096)]),  # multiples of 8 in 0..4096
    19: (1, [(3, 1), (1, 1), (-5, 1), (7, 0), (0, 2), (2, 0), (1, 2)]),     # < 0 -> 0, 3 -> 1, > 2 -> 2
    20: (1, [(0, 1), (7, 0), (0, 1), (-2, 0), (1, 1)]),
    22: (0, [(8, 0), (65, 8), (-1, 8), (0, 8)]),                            # 0..64
    23: (1, [(0, 1), (64, 0), (2, 64), (256, 64), (-1, 64), (128, 64), (1, 128)]),  # 0 / 1 / 64 / 128
    24: (1, [(0, 1), (-1, 0), (300, 0), (1, 300)]),                         # >= 0
    25: (1, [(0, 1), (2, 0), (3, 2), (-1, 2), (1, 2)]),                     # 0..2
    26: (5, [(3, 5), (4, 3), (2, 4), (6, 4), (5, 4)]),                      # 3 / 4 / 5
    27: (1, [(0, 1), (2, 0), (3, 2), (7, 2), (11, 2), (-1, 2), (10, 2), (5, 10), (1, 5)]),  # 0..10 without both low bits
    29: (1, [(0, 1), (2, 0), (3, 2), (-1, 2), (1, 2)]),                     # 0..2
    30: (4, [(0, 4), (2, 0), (12, 0), (-1, 0), (13, 0), (9, 13), (4, 9)]),  # 0 / 1 / 4 / 5 / 8 / 9 / 13
    31: (1, [(2, 1), (10, 2), (11, 2), (3, 2), (-1, 2), (0, 2), (1, 0)]),   # 0..2; 10 / 11 (profile builds) leave it
    32: (1, [(0, 1), (7, 0), (0, 1), (-2, 0), (1, 1)]),
}
UNKNOWN = [0, 16, 17, 21, 33, 99, -1]
NEEDS_DEVICE = {28}  # DRN_TUNE_PP8_PROFILE reads device counters


def check_contract(tune):
    """`tune(knob, value)` = drn_tune of the library under test"""
    for knob, (default, calls) in sorted(CONTRACT.items()):
        restore = calls[-1][0]
        assert tune(knob, restore) == default, "knob %d: default" % knob
        for i, (value, before) in enumerate(calls):
            assert tune(knob, value) == before, "knob %d, call %d: drn_tune(%d, %d)" % (knob, i, knob, value)
        assert tune(knob, restore) == default, "knob %d is back at its default" % knob
        assert tune(knob, restore) == default
    for knob in UNKNOWN:
        for value in (0, 1, -1):
            assert tune(knob, value) == -1, "unknown knob %d" % knob


def test_contract_covers_every_knob():
    assert set(CONTRACT) | NEEDS_DEVICE == set(header_knobs().values())


def test_drn_tune_contract(pkg):
    check_contract(pkg._cabi.lib().drn_tune)


def test_gemm_set_tile_contract(pkg):
    set_tile = pkg._cabi.lib().drn_gemm_set_tile
    for value, before in [(0, 0), (64, 0), (100, 64), (-1, 64), (128, 64), (255, 128), (256, 255), (0, 256), (0, 0)]:
        assert set_tile(value) == before


def test_tuned_restores_in_reverse_order(ops, monkeypatch):
    calls = []
    real = ops.tune

    def spy(knob, value):
        calls.append((knob, value))
        return real(knob, value)

    monkeypatch.setattr(ops, "tune", spy)
    with ops.tuned({ops.TUNE_GEMM_GROUP_ROWS: 8, ops.TUNE_CONV_KS_TILES: 40}) as prev:
        assert prev == {ops.TUNE_GEMM_GROUP_ROWS: 0, ops.TUNE_CONV_KS_TILES: 0}
        assert real(ops.TUNE_GEMM_GROUP_ROWS, 8) == 8 and real(ops.TUNE_CONV_KS_TILES, 40) == 40
    assert calls == [(ops.TUNE_GEMM_GROUP_ROWS, 8), (ops.TUNE_CONV_KS_TILES, 40), (ops.TUNE_CONV_KS_TILES, 0), (ops.TUNE_GEMM_GROUP_ROWS, 0)]
    assert real(ops.TUNE_GEMM_GROUP_ROWS, 0) == 0 and real(ops.TUNE_CONV_KS_TILES, 0) == 0


def test_tuned_restores_on_exception_what_was_there(ops):
    assert ops.tune(ops.TUNE_GEMM_GROUP_ROWS, 16) == 0  # (a non-default setting: tuned puts THAT back, not the default)
    try:
        with pytest.raises(ZeroDivisionError):
            with ops.tuned({ops.TUNE_GEMM_GROUP_ROWS: 8, ops.TUNE_CONV_KS_TILES: 40}, tile=128) as prev:
                assert prev == {"tile": 0, ops.TUNE_GEMM_GROUP_ROWS: 16, ops.TUNE_CONV_KS_TILES: 0}
                1 / 0
        assert ops.gemm_set_tile(0) == 0
        assert ops.tune(ops.TUNE_CONV_KS_TILES, 0) == 0
    finally:
        assert ops.tune(ops.TUNE_GEMM_GROUP_ROWS, 0) == 16


def test_tuned_restores_the_quirky_knobs(ops):
    """what drn_tune returned restores the default state of the two knobs whose return is not simply the stored value"""
    with ops.tuned({ops.TUNE_ROI_LANE: 3}) as prev:  # (3 = lane kernel on, ONE sub-group per walking block)
        assert prev[ops.TUNE_ROI_LANE] == 1
    assert ops.tune(ops.TUNE_ROI_LANE, 1) == 1       # restored with 1: the setting 1 and the default two sub-groups
    with ops.tuned({ops.TUNE_CONV_PATCH: 0}) as prev:
        assert prev[ops.TUNE_CONV_PATCH] == 32768
    assert ops.tune(ops.TUNE_CONV_PATCH, 32768) == 32768  # restored with the threshold: on, threshold unchanged
    with ops.tuned({ops.TUNE_CONV_PATCH: 5000}):
        assert ops.tune(ops.TUNE_CONV_PATCH, 5000) == 5000
    assert ops.tune(ops.TUNE_CONV_PATCH, 32768) == 32768
