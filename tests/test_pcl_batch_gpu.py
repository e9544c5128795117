"""PCL on image batches at the ops level (drn_pcl_adjacency_batch, drn_pcl_refine_batch): every image of a batch, bit for bit,
what the single-image entries give for it alone; the batch loss and the gradient scaling of the definition in
include/drn_wsod.h; the per-image results against oracle/pcl_oracle.py within the bounds of tests/test_pcl_gpu.py; the limits.
Shapes sit where the batch indexing can go wrong (tests/pcl_batch_util.py CASES)."""
import numpy as np
import pytest
import torch

import pcl_batch_util as U
from __graft_entry__ import load_package

pytestmark = pytest.mark.gpu

ROW_KEYS = ("labels", "cls_loss_weights", "gt_assignment")
PC_KEYS = ("pc_labels", "pc_probs", "pc_count", "img_cls_loss_weights", "pc_rows", "pc_scores")
SENTINEL = 7.0
_RUNS = {}


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "GPU tests need a GPU (run with -m gpu on the MI355X box)"
    pkg = load_package()
    pkg._cabi.lib()  # raises if the HIP library is missing: no fallback
    import importlib

    return importlib.import_module("drn_wsod_pytorch_amd.ops")


def _cpu(d):
    return {k: v.cpu() for k, v in d.items()}


def _run(ops, name):
    """the batch through the batch entries and every image alone through the single entries, once per case"""
    if name in _RUNS:
        return _RUNS[name]
    c, images = U.make_case(name)
    K, nb, rows = c["K"], c["nb"], list(c["rows"])
    n, M = len(rows), sum(rows)
    ld, cols = U.layout(K, nb)
    off = [0]
    for r in rows:
        off.append(off[-1] + r)

    def logits_of(img):
        lg = torch.zeros((img["boxes"].shape[0], ld), dtype=torch.float32)
        for b, l in enumerate(img["logits"]):
            lg[:, cols[b]: cols[b] + K + 1] = torch.from_numpy(l)
        return lg

    single = []
    for img in images:
        R = img["boxes"].shape[0]
        bx = torch.from_numpy(img["boxes"]).cuda()
        adj = ops.pcl_adjacency(bx, 0.4)
        dl = torch.full((R, ld), SENTINEL, dtype=torch.float32, device="cuda")
        out = ops.pcl_refine(logits_of(img).cuda(), cols, K, torch.from_numpy(img["last"]).cuda(), bx, adj,
                             torch.from_numpy(img["im"]).cuda(), dl)
        torch.cuda.synchronize()
        single.append(dict(out=[_cpu(o) for o in out], dl=dl.cpu(), adj=adj.cpu()))

    boxes = torch.from_numpy(np.concatenate([i["boxes"] for i in images])).cuda()
    last = torch.from_numpy(np.concatenate([i["last"] for i in images])).cuda()
    lg = torch.cat([logits_of(i) for i in images]).cuda()
    onehot = torch.from_numpy(np.stack([i["im"] for i in images])).cuda()
    img_off = torch.tensor(off, dtype=torch.int32)  # on the host: checked there, then uploaded
    max_rows = max(rows)
    adj = ops.pcl_adjacency_batch(boxes, img_off, n, max_rows, 0.4)
    dl = torch.full((M + 3, ld), SENTINEL, dtype=torch.float32, device="cuda")  # three rows no image owns
    per_image, loss_img, loss = ops.pcl_refine_batch(lg, cols, K, last, boxes, adj, onehot, img_off, n, max_rows, dl)
    torch.cuda.synchronize()
    res = dict(c=c, images=images, cols=cols, ld=ld, off=off, single=single, adj=adj.cpu(), dl=dl.cpu(),
               per_image=[[_cpu(o) for o in p] for p in per_image], loss_img=loss_img.cpu(), loss=loss.cpu())
    _RUNS[name] = res
    return res


def _same(a, b):
    """bit for bit (NaN == NaN: the mean probability of an empty cluster)"""
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


@pytest.mark.parametrize("name", ["uneven3", "edges3", "max2", "four", "eight", "one"])
def test_batch_equals_single_bit_for_bit(ops, name):
    r = _run(ops, name)
    c, off, cols = r["c"], r["off"], r["cols"]
    K, nb, n = c["K"], c["nb"], len(c["rows"])
    scale = np.float32(1.0) / np.float32(n)
    for i in range(n):
        s = r["single"][i]
        for b in range(nb):
            got, want = r["per_image"][i][b], s["out"][b]
            npc = int(want["n_pc"])
            assert torch.equal(got["n_pc"], want["n_pc"]), (name, i, b)
            for k in ROW_KEYS + ("probs",):
                assert _same(got[k], want[k]), (name, i, b, k)
            for k in PC_KEYS:
                assert _same(got[k][:npc], want[k][:npc]), (name, i, b, k)
            if npc:  # row indices are local to the image
                assert int(got["pc_rows"][:npc].max()) < c["rows"][i] and int(got["gt_assignment"].max()) < npc
            assert _same(got["loss"], want["loss"]) and _same(r["loss_img"][i, b: b + 1], want["loss"]), (name, i, b)
            # dlogits: the single-image rows, multiplied once more in float32 by 1.f / n (exact for n = 2, 4, 8; n = 1: equal)
            mine = r["dl"][off[i]: off[i + 1], cols[b]: cols[b] + K + 1]
            alone = s["dl"][:, cols[b]: cols[b] + K + 1]
            assert _same(mine, alone * torch.tensor(scale)), (name, i, b)
            if n in (2, 4, 8):
                assert _same(mine * float(n), alone), (name, i, b)
    # columns no branch owns and rows no image owns are not written
    owned = torch.zeros(r["ld"], dtype=torch.bool)
    for b in range(nb):
        owned[cols[b]: cols[b] + K + 1] = True
    assert torch.all(r["dl"][:, ~owned] == SENTINEL) and torch.all(r["dl"][off[-1]:] == SENTINEL), name
    assert not torch.any(r["dl"][: off[-1], owned] == SENTINEL), name
    # the batch loss: the defined fp64 mean of the per-image losses, in ascending order, rounded once
    assert np.array_equal(r["loss"].numpy(), U.batch_mean(r["loss_img"].numpy())), name


@pytest.mark.parametrize("name", ["uneven3", "edges3", "max2", "eight"])
def test_batch_adjacency_equals_single_and_tails_are_zero(ops, name):
    r = _run(ops, name)
    rows, off = r["c"]["rows"], r["off"]
    W = (max(rows) + 31) // 32
    assert r["adj"].shape == (off[-1], W)
    cols = np.arange(W * 32)
    for i, R in enumerate(rows):
        mine = r["adj"][off[i]: off[i + 1]].numpy().view(np.uint32)
        alone = r["single"][i]["adj"].numpy().view(np.uint32)
        wi = (R + 31) // 32
        assert np.array_equal(mine[:, :wi], alone), (name, i)
        bits = ((mine[:, :, None] >> np.arange(32, dtype=np.uint32)) & 1).reshape(R, -1).astype(bool)
        assert not bits[:, cols >= R].any(), (name, i)  # bits beyond R_i in the last word and every further word


@pytest.mark.parametrize("name", ["uneven3", "edges3", "max2", "eight"])
def test_batch_against_oracle_per_image(ops, name):
    """integers exact, weights / loss / gradient within the bounds of tests/test_pcl_gpu.py (restated in pcl_batch_util);
    the oracle's next branch is fed the device's own probabilities, as there"""
    r = _run(ops, name)
    c, off, cols = r["c"], r["off"], r["cols"]
    K, nb, n = c["K"], c["nb"], len(c["rows"])
    override = [[r["per_image"][i][b]["probs"].numpy() for b in range(nb)] for i in range(n)]
    ref = U.batch_oracle(r["images"], override)
    for i in range(n):
        for b in range(nb):
            o = {k: v.numpy() for k, v in r["per_image"][i][b].items()}
            loss, _, probs, t = ref["per_image"][i][b]
            tag = (name, i, b)
            npc = int(o["n_pc"][0])
            assert npc == len(t["pc_labels"]), tag
            np.testing.assert_allclose(o["probs"], probs, rtol=U.RTOL_PROBS, atol=U.ATOL_PROBS)
            for k, tk in (("labels", "labels"), ("gt_assignment", "gt_assignment"), ("cls_loss_weights", "cls_loss_weights")):
                assert np.array_equal(o[k], t[tk]), tag + (k,)
            for k, tk in (("pc_labels", "pc_labels"), ("pc_count", "pc_count"), ("pc_rows", "centre_rows")):
                assert np.array_equal(o[k][:npc], t[tk]), tag + (k,)
            np.testing.assert_allclose(o["pc_probs"][:npc], t["pc_probs"], rtol=U.RTOL_PC, equal_nan=True)
            np.testing.assert_allclose(o["img_cls_loss_weights"][:npc], t["img_cls_loss_weights"], rtol=U.RTOL_PC)
            got = float(o["loss"][0])
            assert np.isfinite(got) and abs(got - float(loss)) <= U.RTOL_LOSS * max(1.0, abs(float(loss))), tag + (got, loss)
            np.testing.assert_allclose(r["dl"][off[i]: off[i + 1], cols[b]: cols[b] + K + 1].numpy(), ref["dlogits"][i][b],
                                       rtol=U.RTOL_DLOGITS, atol=U.ATOL_DLOGITS / n)
    if 0 in c["labels"]:  # the image without labels: no centres, loss 0, zero gradient (oracle/pcl_oracle.py)
        i = c["labels"].index(0)
        assert r["loss_img"][i].tolist() == [0.0] * nb
        assert all(int(r["per_image"][i][b]["n_pc"]) == 0 for b in range(nb))
    # batch loss against the definition on the oracle's per-image losses: the bound of one image's loss
    for b in range(nb):
        want = float(ref["loss"][b])
        assert abs(float(r["loss"][b]) - want) <= U.RTOL_LOSS * max(1.0, abs(want)), (name, b)


def test_limits_refused_without_a_launch(ops):
    from drn_wsod_pytorch_amd._cabi import DrnError

    off = lambda *o: torch.tensor(o, dtype=torch.int32)
    big = torch.zeros((4097 + 10, 4), device="cuda")
    for dev in ("cpu", "cuda"):  # R_0 = 4097: above the per-image limit, wherever img_off lives
        with pytest.raises(DrnError):
            ops.pcl_adjacency_batch(big, off(0, 4097, 4107).to(dev), 2, 4097, 0.4)
    small = torch.zeros((68, 4), device="cuda")
    with pytest.raises(DrnError):  # more images than DRN_PCL_MAX_IMAGES
        ops.pcl_adjacency_batch(small, off(*range(0, 72, 4)).cuda(), 17, 4, 0.4)
    with pytest.raises(DrnError):  # max_rows below an actual R_i: refused on the host, where the sizes are known
        ops.pcl_adjacency_batch(small, off(0, 10, 68), 2, 40, 0.4)
    with pytest.raises(DrnError):  # ... and what the entry itself can see without the sizes: M > n_img * max_rows
        ops.pcl_adjacency_batch(small, off(0, 10, 68).cuda(), 2, 30, 0.4)
    K, nb = 5, 2
    ld, cols = U.layout(K, nb)
    z = lambda *s: torch.zeros(s, device="cuda")
    dl = torch.full((68, ld), SENTINEL, device="cuda")
    for img_off, n, max_rows in ((off(0, 10, 68), 2, 40), (off(0, 10, 68).cuda(), 2, 30), (off(*range(0, 72, 4)).cuda(), 17, 4)):
        with pytest.raises(DrnError):
            ops.pcl_refine_batch(z(68, ld), cols, K, z(68, K), small, torch.zeros((68, (max_rows + 31) // 32), dtype=torch.int32,
                                                                                  device="cuda"),
                                 z(n, K), img_off, n, max_rows, dl)
    torch.cuda.synchronize()
    assert torch.all(dl == SENTINEL)


def test_device_side_row_bound_skips_the_image(ops):
    """img_off on the device is not read back: an image above max_rows that the host checks cannot see (M <= n_img * max_rows)
    is skipped by both launches - its loss is NaN, so is the batch loss, none of its rows is written - and its neighbour is whole"""
    K, nb, rows = 5, 2, [10, 50]
    images = [U.make_image(R, K, nb, 1, 70 + i) for i, R in enumerate(rows)]
    ld, cols = U.layout(K, nb)
    lg = torch.zeros((60, ld))
    r0 = 0
    for img in images:
        for b, l in enumerate(img["logits"]):
            lg[r0: r0 + len(l), cols[b]: cols[b] + K + 1] = torch.from_numpy(l)
        r0 += len(img["boxes"])
    boxes = torch.from_numpy(np.concatenate([i["boxes"] for i in images])).cuda()
    last = torch.from_numpy(np.concatenate([i["last"] for i in images])).cuda()
    onehot = torch.from_numpy(np.stack([i["im"] for i in images])).cuda()
    off = torch.tensor([0, 10, 60], dtype=torch.int32, device="cuda")
    adj = ops.pcl_adjacency_batch(boxes, off, 2, 40, 0.4)
    dl = torch.full((60, ld), SENTINEL, device="cuda")
    per_image, loss_img, loss = ops.pcl_refine_batch(lg.cuda(), cols, K, last, boxes, adj, onehot, off, 2, 40, dl, rows=rows)
    torch.cuda.synchronize()
    assert torch.isnan(loss_img[1]).all() and torch.isnan(loss).all() and torch.isfinite(loss_img[0]).all()
    assert torch.all(dl[10:] == SENTINEL) and int(per_image[1][0]["n_pc"]) == 0
    b0 = boxes[:10].contiguous()
    dl0 = torch.full((10, ld), SENTINEL, device="cuda")
    alone = ops.pcl_refine(lg[:10].cuda(), cols, K, last[:10].contiguous(), b0, ops.pcl_adjacency(b0, 0.4), onehot[0], dl0)
    for b in range(nb):
        assert torch.equal(per_image[0][b]["labels"], alone[b]["labels"]) and torch.equal(loss_img[0, b: b + 1], alone[b]["loss"])
        assert torch.equal(dl[:10, cols[b]: cols[b] + K + 1] * 2.0, dl0[:, cols[b]: cols[b] + K + 1])
