"""CSC on image batches, the four batch ops: bit for bit against today's single-image ops on each image's slice
(include/drn_wsod.h, "CSC on image batches").  3 images of 1100 / 37 / 200 rows (above and below one 1024-thread sweep, uneven
offsets) and 64x301 / 37x53 / 50x300 pixels padded to 64x301 (W > 256: more than one pixel per thread in the row scan);
K = 20 and K = 80 (both lane layouts of the loss kernel); mean_loss both ways."""
import ctypes
import importlib

import numpy as np
import pytest
import torch

from __graft_entry__ import load_package
from oracle import wsod_oracle as O

pytestmark = pytest.mark.gpu

load_package()
DEV = "cuda"
ROWS = (1100, 37, 200)
SIZES = ((64, 301), (37, 53), (50, 300))
HMAX, WMAX = 64, 301
OFF = (0, 1100, 1137, 1337)
M = OFF[-1]
THIRD = np.float32(1.0) / np.float32(3.0)


@pytest.fixture(scope="module")
def drn():
    return importlib.import_module("drn_wsod_pytorch_amd.ops")


_CACHE = {}


def _mil(drn, K):
    """logits [M, 2K], labels [3, K] and the batch's MIL scores / row softmax, made once per K and never modified"""
    if K not in _CACHE:
        rs = np.random.RandomState(100 + K)
        logits = torch.from_numpy((rs.randn(M, 2 * K) * 2).astype(np.float32)).to(DEV)
        oh = torch.zeros((3, K))
        for i in range(3):
            oh[i, rs.permutation(K)[: 1 + i]] = 1
        oh = oh.to(DEV)
        off = torch.tensor(OFF, dtype=torch.int32, device=DEV)
        scores, _, _, rowsm = drn.wsddn_fwd_bwd(logits, 0, K, K, off, 3, oh, max_rows=max(ROWS), return_rowsm=True)
        Wt = torch.from_numpy((rs.rand(M, K) * 2.2 - 1.2).astype(np.float32)).clamp(-1, 1).to(DEV)
        _CACHE[K] = dict(logits=logits, oh=oh, off=off, scores=scores, rowsm=rowsm, W=Wt)
    return _CACHE[K]


def _rois(rs, n, H, W, img):
    """tests/test_csc_gpu.py::_rois with the image index in column 0: boxes partly outside the image, .5 corners"""
    x0 = rs.rand(n) * (W + 8) - 4
    y0 = rs.rand(n) * (H + 8) - 4
    b = np.stack([np.full(n, img), x0, y0, x0 + rs.rand(n) * W * 0.9 + 1, y0 + rs.rand(n) * H * 0.9 + 1], 1).astype(np.float32)
    b[: n // 8, 1:] = np.round(b[: n // 8, 1:]) + 0.5
    return b


@pytest.mark.parametrize("K", [20, 80])
def test_seed_batch_bit_equal_per_image(drn, K):
    d = _mil(drn, K)
    slot = (3, -1, 0)
    dl = torch.full((M, 2 * K), 7.0, dtype=torch.float32, device=DEV)
    drn.csc_seed_batch(d["logits"], 0, K, K, d["scores"], d["rowsm"], d["off"], 3, torch.tensor(slot, device=DEV), dl)
    for i, c in enumerate(slot):
        a, b = OFF[i], OFF[i + 1]
        if c < 0:
            assert not dl[a:b].any()  # exactly zero: the batched d/dx pass carries nothing for this image
            continue
        want = torch.full((b - a, 2 * K), 7.0, dtype=torch.float32, device=DEV)
        drn.csc_loss(d["logits"][a:b], 0, K, K, d["scores"][a:b], d["rowsm"][a:b], None, None, False, dlogits=want, seed_class=c)
        assert torch.equal(dl[a:b], want), (i, c)
        assert float(want.abs().max()) > 0


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_cpg_batch_reads_only_the_crop(drn, dtype):
    K, slot = 20, (3, -1, 0)
    rs = np.random.RandomState(11)
    cp = 8 if dtype == torch.bfloat16 else 4
    g = torch.from_numpy(rs.randn(3, HMAX, WMAX, cp).astype(np.float32))
    g[..., 3:] = 1e6                       # channel padding
    for i, (H, W) in enumerate(SIZES):     # the padding region of the batch tensor
        g[i, H:] = 1e6
        g[i, :, W:] = 1e6
    g = g.to(dtype).to(DEV).contiguous()
    plan = drn.CscBatchPlan(SIZES, K, [list(slot)], [], DEV)
    flat = torch.full((plan.map_floats,), 0.25, dtype=torch.float32, device=DEV)
    drn.csc_cpg_batch(g, 3, plan, 0, flat)
    maps = plan.map_views(flat)
    for i, ((H, W), c) in enumerate(zip(SIZES, slot)):
        for k in range(K):
            if k != c:
                assert bool((maps[i][k] == 0.25).all()), (i, k)  # untouched (an image with -1: every class)
        if c < 0:
            continue
        want = drn.csc_cpg(g[i: i + 1, :H, :W].contiguous(), 3)
        assert torch.equal(maps[i][c], want), i
        assert float(want.max()) == 1.0 and float(want.min()) >= 0.0


def test_weights_batch_bit_equal_per_pair(drn):
    K = 20
    rs = np.random.RandomState(5)
    pairs = [(0, 1), (0, 3), (0, 4), (1, 0), (2, 2), (2, 19)]  # 3 / 1 / 2 classes; (0, 4) keeps a zero map (below tau)
    plan = drn.CscBatchPlan(SIZES, K, [], pairs, DEV)
    flat, maps = plan.new_maps(DEV)
    for i, c in pairs:
        if (i, c) == (0, 4):
            continue
        H, W = SIZES[i]
        yy, xx = np.mgrid[0:H, 0:W]
        cy, cx, s = rs.rand() * H, rs.rand() * W, 0.15 * min(H, W) + 2
        m = np.exp(-((yy - cy) ** 2 + (xx - cx) ** 2) / (2 * s * s)) + 0.08 * rs.rand(H, W)
        m = (m / m.max()).astype(np.float32)
        m[rs.rand(H, W) < 0.05] = np.float32(0.1)  # exactly on the threshold: foreground
        maps[i][c].copy_(torch.from_numpy(m))
    rois = torch.from_numpy(np.concatenate([_rois(rs, r, H, W, i) for i, (r, (H, W)) in enumerate(zip(ROWS, SIZES))])).to(DEV)
    scores = torch.from_numpy((rs.rand(M, K) / 300 * 1.6).astype(np.float32)).to(DEV)
    off = torch.tensor(OFF, dtype=torch.int32, device=DEV)
    Wb = torch.ones((M, K), dtype=torch.float32, device=DEV)
    tables = drn.csc_weights_batch(flat, plan, 0.1, rois, off, scores, True, 1.8, Wb)
    want = torch.ones((M, K), dtype=torch.float32, device=DEV)
    for i, c in pairs:
        a, b = OFF[i], OFF[i + 1]
        Wi = torch.ones((b - a, K), dtype=torch.float32, device=DEV)
        drn.csc_weights(maps[i][c].contiguous(), 0.1, rois[a:b].contiguous(), scores[a:b].contiguous(), c, True, 1.8, Wi)
        want[a:b, c] = Wi[:, c]
    assert torch.equal(Wb, want)
    named = {(i, c) for i, c in pairs}
    for i in range(3):
        for c in range(K):
            if (i, c) not in named:
                assert bool((Wb[OFF[i]: OFF[i + 1], c] == 1).all())  # a column of an unlabelled class stays 1
    assert float(Wb.min()) < -0.5 and not bool((Wb[:, 3] == 1).all())
    # the summed-area table of one pair against the oracle's
    lib = O._lib()
    tv = plan.table_views(tables)
    for p in (1, 3, 5):
        i, c = pairs[p]
        H, W = SIZES[i]
        m = maps[i][c].cpu().contiguous()
        t = torch.empty((H, W), dtype=torch.float32)
        lib.oracle_csc_integral(O._fp(m), O._fp(t), H, W, ctypes.c_float(np.float32(1.0) * np.float32(0.1)))
        assert torch.equal(tv[p].cpu(), t), pairs[p]


@pytest.mark.parametrize("K", [20, 80])
@pytest.mark.parametrize("mean_loss", [False, True])
def test_loss_batch_is_the_mean_of_the_single_image_losses(drn, K, mean_loss):
    d = _mil(drn, K)
    for Wt in (d["W"], None):  # None: past WSL.CSC_MAX_ITER (W = ones), the same mean
        dl = torch.full((M, 2 * K), 7.0, dtype=torch.float32, device=DEV)
        loss_img, loss = drn.csc_loss_batch(d["logits"], 0, K, K, d["scores"], d["rowsm"], Wt, d["oh"], d["off"], 3, mean_loss,
                                            dlogits=dl)
        singles = []
        for i in range(3):
            a, b = OFF[i], OFF[i + 1]
            dli = torch.full((b - a, 2 * K), 7.0, dtype=torch.float32, device=DEV)
            li = drn.csc_loss(d["logits"][a:b], 0, K, K, d["scores"][a:b], d["rowsm"][a:b], None if Wt is None else Wt[a:b],
                              d["oh"][i], mean_loss, dlogits=dli)
            assert torch.equal(loss_img[i], li), (i, loss_img[i], li)
            got, want = dl[a:b].cpu().numpy(), (dli.cpu().numpy() * THIRD).astype(np.float32)
            assert np.array_equal(got, want), i
            singles.append(li.cpu().numpy())
        for j in range(2):
            l0, l1, l2 = (s[j] for s in singles)
            want = np.float32((np.float64(l0) + np.float64(l1) + np.float64(l2)) / 3)
            print("K %d mean_loss %s W %s loss[%d]: batch %.9g singles %.9g %.9g %.9g" % (
                K, mean_loss, Wt is not None, j, float(loss[j]), l0, l1, l2))
            assert np.float32(loss[j].cpu().numpy()) == want, (j, float(loss[j]), want)
        assert np.isfinite(loss.cpu().numpy()).all() and float(loss[0]) > 0
