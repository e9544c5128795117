"""CPU test of the RoIPool forward's kernel choice as drn_roi_pool_workspace_bytes reports it (the query is host-only: it asks
roi_fwd_plan for the plan of the best case - no out_t, everything aligned - and returns the bytes that plan pools from).
The table was recorded from the library as it was before the choice moved into one plan; the same table has to pass against
any later build."""
import importlib

import pytest

from __graft_entry__ import build

BF16, F32 = 1, 0


@pytest.fixture(scope="module")
def ops():
    build()
    return importlib.import_module("drn_wsod_pytorch_amd.ops")


# (N, H, W, C, M) -> bytes under: default | ROI_ST = 0 | ROI_ST = 2 | ROI_LANE = 0 | ROI_LANE = 2 | ROI_LANE = 3
# (bf16, P = 7, RoIPool, no arg-max).  0: a kernel that takes no workspace (lane, 64-ROI, 8-ROI); N*H*W*C*2: the walking kernel's
# chunk-major copy; that plus a 256-byte record and a class byte per ROI (each part rounded up to 256): the sparse table.
# The shapes are those of tests/test_ops_gpu.py's RoIPool cases and BASELINE's real-image sizes, plus the two sides of every
# threshold of the default rule (M = 600 / 1500 / 400, 3000 / 1800 cells, the 38-KB slice, 255 columns, 10 images, 16384 ROIs).
TABLE = {
    (1, 14, 14, 1024, 2000): (0, 0, 915456, 0, 0, 0),
    (1, 50, 76, 1024, 2000): (8296448, 7782400, 8296448, 0, 8296448, 8296448),
    (1, 99, 151, 2048, 2000): (61745152, 0, 61745152, 0, 61745152, 61745152),
    (2, 63, 92, 128, 300): (2967552, 2967552, 3044864, 0, 0, 2967552),
    (1, 150, 200, 256, 3000): (16131072, 0, 16131072, 0, 16131072, 16131072),
    (3, 43, 58, 64, 150): (957696, 957696, 996352, 0, 0, 957696),
    (1, 30, 40, 16, 64): (0, 0, 55040, 0, 0, 0),
    (1, 75, 122, 16, 130): (292800, 292800, 326400, 0, 0, 292800),
    (2, 14, 14, 64, 200): (0, 0, 101632, 0, 0, 0),
    (2, 50, 76, 128, 130): (1945600, 1945600, 1979136, 0, 0, 1945600),
    (3, 14, 14, 128, 83): (0, 0, 172032, 0, 0, 0),
    (2, 28, 28, 64, 200): (0, 0, 252160, 0, 0, 0),
    (2, 50, 76, 128, 300): (1945600, 1945600, 2022912, 0, 0, 1945600),
    (2, 63, 92, 16, 130): (370944, 370944, 404480, 0, 0, 370944),
    (4, 40, 37, 24, 65): (284160, 284160, 301056, 0, 0, 284160),
    (2, 14, 14, 64, 100): (0, 0, 76032, 0, 0, 0),
    (2, 99, 151, 64, 140): (0, 0, 3863040, 0, 0, 0),
    (3, 63, 92, 128, 300): (4451328, 4451328, 4528640, 0, 0, 4451328),
    (2, 23, 29, 128, 80): (0, 0, 362240, 0, 0, 0),
    (2, 40, 37, 64, 80): (378880, 378880, 399616, 0, 0, 378880),
    (2, 43, 58, 64, 64): (638464, 638464, 655104, 0, 0, 638464),
    (2, 99, 151, 64, 400): (3929856, 0, 3929856, 0, 3929856, 3929856),
    (1, 118, 160, 16, 400): (707072, 0, 707072, 0, 707072, 707072),
    (3, 70, 255, 8, 400): (959744, 0, 959744, 0, 959744, 959744),
    (1, 50, 76, 16, 640): (286208, 121600, 286208, 0, 286208, 286208),
    (2, 150, 200, 8, 400): (1062912, 0, 1062912, 0, 1062912, 1062912),
    (1, 140, 145, 8, 400): (427776, 0, 427776, 0, 427776, 427776),
    (10, 81, 101, 8, 120): (1308960, 1308960, 1340160, 0, 0, 1308960),
    (2, 63, 92, 32, 300): (741888, 741888, 819200, 0, 0, 741888),
    (3, 43, 58, 64, 200): (957696, 957696, 1009152, 0, 0, 957696),
    (1, 50, 76, 1024, 599): (7782400, 7782400, 7936512, 0, 0, 7782400),
    (1, 50, 76, 1024, 600): (7936768, 7782400, 7936768, 0, 7936768, 7936768),
    (1, 43, 58, 1024, 1499): (5107712, 5107712, 5492992, 0, 0, 5107712),
    (1, 43, 58, 1024, 1500): (5493248, 5107712, 5493248, 0, 5493248, 5493248),
    (1, 42, 43, 256, 2000): (1438720, 924672, 1438720, 0, 1438720, 1438720),
    (1, 99, 151, 64, 399): (0, 0, 2016256, 0, 0, 0),
    (1, 38, 38, 256, 2000): (739328, 739328, 1253376, 0, 0, 739328),
    (1, 48, 50, 512, 2000): (2971648, 2457600, 2971648, 0, 2971648, 2971648),
    (1, 101, 102, 512, 1000): (10806272, 0, 10806272, 0, 10806272, 10806272),
    (1, 181, 182, 64, 1000): (0, 0, 0, 0, 0, 0),
    (1, 256, 100, 64, 1000): (0, 0, 0, 0, 0, 0),
    (11, 50, 76, 64, 2000): (5350400, 5350400, 5350400, 0, 0, 5350400),
    (1, 50, 76, 1024, 16385): (7782400, 7782400, 7782400, 0, 0, 7782400),
    (1, 75, 100, 24, 2000): (874240, 360000, 874240, 0, 874240, 874240),
    (1, 75, 122, 1024, 1500): (19124736, 18739200, 19124736, 0, 19124736, 19124736),
}
STATES = ["default", "ROI_ST=0", "ROI_ST=2", "ROI_LANE=0", "ROI_LANE=2", "ROI_LANE=3"]


def _knobs(ops, state):
    if state == "default":
        return {}
    name, val = state.split("=")
    return {getattr(ops, "TUNE_" + name): int(val)}


def _query(ops, shape, P=7, mode=0, argmax=0, din=BF16, dout=BF16):
    n, h, w, c, m = shape
    return ops.C.lib().drn_roi_pool_workspace_bytes(n, h, w, c, P, m, mode, argmax, din, dout)


@pytest.mark.parametrize("col", range(len(STATES)), ids=STATES)
def test_workspace_bytes_table(ops, col):
    with ops.tuned(_knobs(ops, STATES[col])):
        got = {s: _query(ops, s) for s in TABLE}
    assert got == {s: row[col] for s, row in TABLE.items()}


def test_table_covers_every_class():
    """at least 15 shapes each of: no workspace, the walking kernel's copy, the sparse table's workspace"""
    cells = [(s, b) for s, row in TABLE.items() for b in row]
    none = {s for s, b in cells if b == 0}
    walk = {s for s, b in cells if b == s[0] * s[1] * s[2] * s[3] * 2}
    table = {s for s, b in cells if b > s[0] * s[1] * s[2] * s[3] * 2}
    assert all(b == 0 or b >= s[0] * s[1] * s[2] * s[3] * 2 for s, b in cells)
    assert min(len(none), len(walk), len(table)) >= 15, (len(none), len(walk), len(table))


@pytest.mark.parametrize("state", STATES)
def test_rejected_cases_need_no_workspace(ops, state):
    """ROIAlign, P != 7, arg-max wanted, fp32 on either side, fewer than 64 ROIs, C not a multiple of 8, an empty shape: 0
    whatever the knobs say"""
    big = (1, 50, 76, 1024, 2000)  # 8296448 bytes under the default
    with ops.tuned(_knobs(ops, state)):
        assert _query(ops, big, mode=1) == 0
        assert _query(ops, big, P=6) == 0 and _query(ops, big, P=8) == 0
        assert _query(ops, big, argmax=1) == 0
        assert _query(ops, big, din=F32, dout=F32) == 0 and _query(ops, big, din=F32) == 0 and _query(ops, big, dout=F32) == 0
        assert _query(ops, (1, 50, 76, 1024, 63)) == 0
        assert _query(ops, (1, 50, 76, 1020, 2000)) == 0 and _query(ops, (1, 50, 76, 1028, 2000)) == 0
        for bad in ((0, 50, 76, 1024, 2000), (1, 0, 76, 1024, 2000), (1, 50, 0, 1024, 2000), (1, 50, 76, 0, 2000)):
            assert _query(ops, bad) == 0
