"""drn_csc_stats on the device against the numpy restatement of tests/csc_stats_util.py (fp64 / int64).  Integer fields are exact.
Every row sum is one fp64 chain over at most a few thousand rows - its error is far below fp32's half-ulp - rounded to fp32
once, so a contribution is within ONE fp32 spacing of the fp64 value, and a table sum within the sum of its contributions'
spacings (U.assert_close; the bound is computed from the restatement, never from the kernel).
Shapes: K in {1, 20, 65, 128} (one / two waves of column threads; 4096 / K rows per LDS tile = 4096, 204, 63, 32), rows per image
in {1, 63, 64, 65, 257} (below, at and across a tile edge for K = 65 and 128; 257 crosses it for K = 20), n_img in {1, 3} with
unequal row counts; K = 1 with 4100 rows crosses its only tile edge."""
import numpy as np
import pytest
import torch

import csc_stats_util as U
from __graft_entry__ import load_package

load_package()
from drn_wsod_pytorch_amd import metrics, ops  # noqa: E402

pytestmark = pytest.mark.gpu

ROWS = (1, 63, 64, 65, 257)
BATCHES = ((1, 63, 257), (64, 65, 63), (257, 1, 64))


def _slots(active, n_img):
    """the slot rows of a set of (image, class): slot j carries the j-th active class of every image, -1 where it has fewer"""
    per = [sorted(c for i, c in active if i == k) for k in range(n_img)]
    S = max([len(a) for a in per] + [0])
    return [[a[j] if j < len(a) else -1 for a in per] for j in range(S)]


def _case(rng, rows, K, empty=None, pattern=True):
    """scores with column sums below 1, W columns by c % 4: all positive, all negative, all +0.0 / -0.0, mixed with zeros and a
    NaN; random labels (image `empty`: none), a random part of the labelled classes active"""
    n, M = len(rows), sum(rows)
    off = np.concatenate([[0], np.cumsum(rows)]).astype(np.int32)
    scores = (rng.random((M, K)) / np.repeat(rows, rows)[:, None] * 1.6).astype(np.float32)
    W = rng.uniform(-1, 1, (M, K)).astype(np.float32)
    if pattern:
        for c in range(K):
            if c % 4 == 0:
                W[:, c] = np.abs(W[:, c]) + np.float32(1e-3)
            elif c % 4 == 1:
                W[:, c] = -np.abs(W[:, c]) - np.float32(1e-3)
            elif c % 4 == 2:
                W[:, c] = np.where(rng.random(M) < 0.5, np.float32(0.0), np.float32(-0.0))
            else:
                W[rng.random(M) < 0.3, c] = 0.0
                W[rng.random(M) < 0.05, c] = np.nan
    onehot = (rng.random((n, K)) < 0.6).astype(np.float32)
    onehot[:, -1] = 1.0
    if empty is not None:
        onehot[empty] = 0.0
    active = {(i, c) for i in range(n) for c in range(K) if onehot[i, c] > 0.5 and rng.random() < 0.7}
    if K > 1:
        active.discard((0, K - 1))  # a labelled, inactive class
    return dict(scores=scores, W=W, off=off, onehot=onehot, active=active, n=n, K=K)


def _launch(case, table, scratch=None):
    dev = "cuda"
    sl = _slots(case["active"], case["n"])
    slots = torch.tensor(sl, dtype=torch.int64, device=dev).reshape(-1) if sl else None
    ops.csc_stats(torch.from_numpy(case["scores"]).to(dev), torch.from_numpy(case["W"]).to(dev),
                  torch.from_numpy(case["off"]).to(dev), case["n"], torch.from_numpy(case["onehot"]).to(dev), slots, table, scratch)


def _ref(cases, K, **kw):
    t = U.new_table(K)
    for c in cases:
        U.add_step(t, c["scores"], c["W"], c["off"], c["onehot"], c["active"], round32=False, **kw)
    return t


def _table(K):
    return torch.zeros((ops.csc_stats_words(K),), dtype=torch.int64, device="cuda")


def _read(table, K):
    torch.cuda.synchronize()
    return metrics.decode_csc_stats(table.cpu().numpy(), K)


@pytest.mark.parametrize("K", [1, 20, 65, 128])
def test_single_image_every_row_count(K):
    rng = np.random.default_rng(100 + K)
    for R in ROWS + ((4100,) if K == 1 else ()):
        case = _case(rng, [R], K)
        table = _table(K)
        _launch(case, table)
        U.assert_close(_read(table, K), _ref([case], K), "K %d R %d" % (K, R))


@pytest.mark.parametrize("K", [1, 20, 65, 128])
def test_three_images_unequal_rows(K):
    """image 1 has no labelled class; (0, K - 1) is labelled and inactive; the columns run through all four weight patterns"""
    rng = np.random.default_rng(200 + K)
    for rows in BATCHES:
        case = _case(rng, list(rows), K, empty=1)
        assert case["onehot"][1].sum() == 0 and (K == 1 or (case["onehot"][0, K - 1] > 0.5 and (0, K - 1) not in case["active"]))
        table = _table(K)
        _launch(case, table)
        got, ref = _read(table, K), _ref([case], K)
        U.assert_close(got, ref, "K %d rows %s" % (K, rows))
        assert got["num_img"] == 3 and got["steps"] == 1
        if K >= 4:
            act = [c for c in range(K) if got["csc_label"][c] > 0]
            for c in act:
                n = got["csc_num_roi"][c]
                want = {0: (n, 0, 0), 1: (0, n, 0), 2: (0, 0, n)}.get(c % 4)
                if want is not None:
                    assert (got["csc_roi_pos"][c], got["csc_roi_neg"][c], got["csc_roi_zero"][c]) == want, c
            assert {c % 4 for c in act} == {0, 1, 2, 3}


def test_invalid_row_ranges_skip_the_image_whole():
    """an empty range and a range that ends past M: nothing of those images is counted, not even num_img, and nothing is read
    outside the tensors (the ranges are checked before any row is touched)"""
    K = 20
    rng = np.random.default_rng(5)
    case = _case(rng, [5, 7, 4], K)
    for off in ([0, 5, 5, 16], [0, 5, 12, 19], [0, 5, 3, 16]):
        bad = dict(case, off=np.array(off, np.int32))
        table = _table(K)
        _launch(bad, table)
        got = _read(table, K)
        U.assert_close(got, _ref([bad], K, M=16), "img_off %s" % off)
        assert got["num_img"] == 2


def test_launches_accumulate_drain_rearms_and_bits_repeat():
    K = 20
    rng = np.random.default_rng(9)
    cases = [_case(rng, list(r), K) for r in ((65, 257), (64,), (1, 63, 257))]
    st = metrics.CscStats(K, 10 ** 6, 10 ** 6, None, "", 1, "cuda")
    for c in cases:
        _launch(c, st.table, st.scratch)
    three = _read(st.table, K)
    U.assert_close(three, _ref(cases, K), "three launches")
    singles = []
    for c in cases:
        t = _table(K)
        _launch(c, t)
        singles.append(_read(t, K))
    for f in U.INT_FIELDS:  # the sum of the three tables
        assert np.array_equal(three[f], singles[0][f] + singles[1][f] + singles[2][f]), f
    for f in U.FP_FIELDS:   # (fp64 adds of the same three values per class in the same order: exact)
        assert np.array_equal(three[f], (singles[0][f] + singles[1][f]) + singles[2][f]), f
    assert three["steps"] == 3 and three["num_img"] == 6
    # drain: the copy holds the table, the table is zero again, the next launch starts clean
    st.drain(3)
    (it, drained), = st.collect(wait=True)
    assert it == 3
    for k, v in three.items():
        assert np.array_equal(drained[k], v), k
    assert not bool(st.table.any())
    _launch(cases[1], st.table, st.scratch)
    again = _read(st.table, K)
    for k, v in singles[1].items():
        assert np.array_equal(again[k], v), k
    # the same inputs twice: the same bits
    a, b = _table(K), _table(K)
    _launch(cases[2], a)
    _launch(cases[2], b)
    torch.cuda.synchronize()
    assert torch.equal(a, b) and bool(a.any())
