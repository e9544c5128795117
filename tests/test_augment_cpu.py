"""The host half of the device data path (DatasetMapper(cfg, is_train, device=...).plan), without a GPU: plan() + the plain-numpy
restatement of drn_augment_u8's arithmetic (tests/augment_util.py) reproduce the reference's own DatasetMapper output
(tests/golden/data_mapper.npz) bit for bit, plan() draws from np.random exactly as the host path does, its result pickles and
travels through loader workers, and a mapper without a device behaves as before."""
import pickle

import numpy as np
import torch

import augment_util as A
from __graft_entry__ import load_package

load_package()
from drn_wsod_pytorch_amd import data as D  # noqa: E402

CASES = (("train", True, 4), ("test", False, 1))


def test_restatement_of_plan_reproduces_the_reference_images(tmp_path):
    """the specification: plan()'s "image_src" + "aug" through the restated arithmetic == train0..3_image and test0_image"""
    d, cfg, recs = A.golden_record(tmp_path)
    for tag, is_train, nrep in CASES:
        mapper = D.DatasetMapper(cfg, is_train, device="cuda")
        np.random.seed(int(d["seed"]))
        for rep in range(nrep):
            p = mapper.plan(recs[0])
            k = "%s%d_" % (tag, rep)
            src = p["image_src"]
            assert src.dtype == torch.uint8 and src.is_contiguous() and src.shape == d["rgb"].shape
            got = A.restate(src.numpy(), p["aug"])
            assert got.shape == d[k + "image"].shape, k
            assert int((got != d[k + "image"]).sum()) == 0, k


def test_plan_equals_the_host_path(tmp_path):
    d, cfg, recs = A.golden_record(tmp_path)
    for tag, is_train, nrep in CASES:
        mapper = D.DatasetMapper(cfg, is_train, device="cuda")
        np.random.seed(int(d["seed"]))
        for rep in range(nrep):
            p = mapper.plan(recs[0])
            k = "%s%d_" % (tag, rep)
            assert "image" not in p
            A.assert_boxes_equal_golden(p, d, k, is_train)
            assert tuple(p["aug"]["out_hw"]) == d[k + "image"].shape[1:], k
            assert p["proposals"].image_size == d[k + "image"].shape[1:], k
            for v in list(p["aug"]["crop"]) + list(p["aug"]["out_hw"]):
                assert type(v) is int
            assert type(p["aug"]["flip"]) is bool
            for name in ("wb", "ws"):
                assert (type(p["aug"][name]) is float) == is_train and (is_train or p["aug"][name] is None)
            if is_train:
                assert 1 / 1.5 <= p["aug"]["wb"] <= 1.5 and 1 / 1.5 <= p["aug"]["ws"] <= 1.5


def test_plan_draws_like_the_host_path(tmp_path):
    d, cfg, recs = A.golden_record(tmp_path)
    states = []
    for device in (None, "cuda"):
        mapper = D.DatasetMapper(cfg, True, device=device)
        np.random.seed(int(d["seed"]))
        for _ in range(4):
            mapper(recs[0]) if device is None else mapper.plan(recs[0])
        states.append(np.random.get_state())
    (n0, k0, p0, h0, c0), (n1, k1, p1, h1, c1) = states
    assert n0 == n1 and np.array_equal(k0, k1) and (p0, h0, c0) == (p1, h1, c1)


def _seed_worker(worker_id):
    np.random.seed(1000 + worker_id)


def _as_is(item):
    return item


def test_plan_is_picklable_gpu_free_and_runs_in_loader_workers(tmp_path, monkeypatch):
    d, cfg, recs = A.golden_record(tmp_path)

    def no_gpu(*a, **k):
        raise AssertionError("plan() must not touch the GPU")

    with monkeypatch.context() as m:
        m.setattr(torch.cuda, "_lazy_init", no_gpu)
        mapper = D.DatasetMapper(cfg, True, device="cuda")
        np.random.seed(5)
        p = mapper.plan(recs[0])
    q = pickle.loads(pickle.dumps(p))
    A.assert_items_equal(p, q)
    for v in p.values():
        assert not (torch.is_tensor(v) and v.is_cuda)
    pickle.loads(pickle.dumps(mapper))  # (a spawned worker receives the mapper itself)
    n = 4
    loader = torch.utils.data.DataLoader(D.MapDataset(recs * n, mapper.plan), batch_size=None, num_workers=2,
                                         worker_init_fn=_seed_worker, collate_fn=_as_is)
    from_workers = list(loader)
    assert len(from_workers) == n
    mine = [None] * n
    for w in range(2):  # worker w maps items w, w + 2, ... in this order
        np.random.seed(1000 + w)
        for i in range(w, n, 2):
            mine[i] = mapper.plan(recs[0])
    assert len({tuple(m["aug"]["crop"]) for m in mine}) > 1  # the draws differ from item to item
    for a, b in zip(from_workers, mine):
        A.assert_items_equal(a, b)


def test_without_a_device_nothing_changes(tmp_path):
    d, cfg, recs = A.golden_record(tmp_path)
    for tag, is_train, nrep in CASES:
        mapper = D.DatasetMapper(cfg, is_train)
        assert mapper.device is None
        np.random.seed(int(d["seed"]))
        for rep in range(nrep):
            out = mapper(recs[0])
            k = "%s%d_" % (tag, rep)
            assert "aug" not in out and "image_src" not in out
            assert out["image"].dtype == torch.uint8 and not out["image"].is_cuda
            assert np.array_equal(out["image"].numpy(), d[k + "image"]), k
            A.assert_boxes_equal_golden(out, d, k, is_train)
    cfg.merge_from_list(["DATALOADER.NUM_WORKERS", "0"])
    np.random.seed(3)
    loader = D.build_detection_train_loader(cfg, recs * 4)
    assert not isinstance(loader, D._DeviceFinishLoader)
    batch = next(iter(loader))
    assert all(x["image"].dtype == torch.uint8 and not x["image"].is_cuda for x in batch)


def _tile_need(n_in, n_out, tile):
    """largest source extent [lo, hi) any tile of `tile` consecutive outputs really reads, from Pillow's own tables"""
    from drn_wsod_pytorch_amd import ops

    if n_in == n_out:
        return min(tile, n_in)
    b, _, _ = ops.pil_bilinear_coeffs(n_in, n_out)
    lo, hi = b[:, 0].astype(np.int64), (b[:, 0] + b[:, 1]).astype(np.int64)
    return max(int(hi[i: i + tile].max() - lo[i: i + tile].min()) for i in range(0, n_out, tile))


def test_lds_bound_covers_every_real_tile_window():
    """drn_augment_u8 sizes its LDS from a host-side bound on a 64 x 16 tile's source window (drn_augment_lds_bytes), and every
    block compares its ACTUAL window with what it was given, taking the per-pixel path where it is larger - same bits, so an
    under-estimating bound would silently leave the staged code unused.  Here: wherever the query promises staging, the bytes
    it asks for cover the largest window any tile really has (from pil_bilinear_coeffs), so the staged path is the one that runs."""
    from drn_wsod_pytorch_amd import ops

    rs = np.random.RandomState(3)
    shapes = [((41, 29), (64, 91)), ((160, 120), (45, 60)), ((60, 50), (173, 60)), ((48, 64), (64, 48)), ((800, 600), (30, 40)),
              ((450, 340), (800, 1059)), ((500, 375), (480, 640)), ((500, 375), (1216, 1621)), ((64, 16), (64, 16)), ((1, 1), (7, 5))]
    for _ in range(300):
        cw, ch = int(rs.randint(1, 700)), int(rs.randint(1, 700))
        f = float(np.exp(rs.uniform(np.log(0.15), np.log(6.0))))
        ho, wo = max(1, int(ch * f * rs.uniform(0.9, 1.1))), max(1, int(cw * f * rs.uniform(0.9, 1.1)))
        shapes.append(((cw, ch), (ho, wo)))
    staged = 0
    for (cw, ch), (ho, wo) in shapes:
        ncols, nrows = _tile_need(cw, wo, 64), _tile_need(ch, ho, 16)
        for c in (1, 3, 4):
            got = ops.augment_u8_lds_bytes((cw, ch), (ho, wo), c)
            need = nrows * (((ncols * c + 6) >> 2) + 64) * 4  # the kernel's own test: rows x (staged dwords + 64 packed pixels) x 4
            if got > 0:
                staged += 1
                assert got >= need, ((cw, ch), (ho, wo), c, got, need)
            else:
                assert need > 16 * 1024, ((cw, ch), (ho, wo), c, need)  # (staging is only given up for windows of real size)
    assert staged > len(shapes)
    assert ops.augment_u8_lds_bytes((800, 600), (30, 40), 3) == 0  # the issue's fallback case
