"""GPU tests of the order-fixed, atomic-free RoIPool / ROIAlign backward (drn_roi_pool_backward_det_nhwc) and of the package's
deterministic mode.  Definition under test (include/drn_wsod.h): every element of dfeat is +0.0f plus its contributions added one
at a time in ascending (ROI, bin[, iy, ix, tap]) order, each rounded to fp32 first - so RoIPool equals the oracle's sequential
scatter bit for bit, both modes decompose bit for bit by image and by channel, and whole training runs repeat bit for bit."""
import numpy as np
import pytest
import torch

import golden_util as G
from __graft_entry__ import load_package

pytestmark = pytest.mark.gpu
O = G.O
DEV = "cuda"
DTYPES = [torch.float32, torch.bfloat16]
P, SCALE, N_IMG = 7, 0.125, 2
# (C, H, W, R): ragged tiles + ragged channel chunk; > 64 ROIs per tile (several ballot rounds); > 1 channel chunk with a tile
# that few or no ROIs reach; and a map large enough that the launcher takes its 8 x 8 tiles (the others run on 4 x 4)
CASES = [(70, 19, 23, 60), (128, 14, 14, 200), (300, 9, 9, 3), (130, 41, 67, 40)]


@pytest.fixture(scope="module")
def drn():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    pkg = load_package()
    pkg._cabi.lib()  # raises if the HIP library is missing: no fallback
    import importlib

    return importlib.import_module("drn_wsod_pytorch_amd.ops")


def _rnd(shape, seed):
    return torch.from_numpy(np.random.RandomState(seed).standard_normal(shape).astype(np.float32))


def _q(x, dtype):
    return x.to(dtype).float()


def _rois(R, H, W, seed):
    """[R, 5] boxes in image coordinates of an (H / SCALE) x (W / SCALE) image; the batch indices interleave (0, 1, 0, 1, ...);
    row 0 lies fully outside the map (empty bins, arg-max -1), row 1 is degenerate (zero size, a .5 rounding case), row 2 covers
    the whole map"""
    rs = np.random.RandomState(seed)
    imw, imh = W / SCALE, H / SCALE
    w, h = 8 + rs.rand(R) * (imw - 8), 8 + rs.rand(R) * (imh - 8)
    x0, y0 = rs.rand(R) * (imw - w), rs.rand(R) * (imh - h)
    r = np.stack([np.arange(R) % N_IMG, x0, y0, x0 + w, y0 + h], 1)
    r[0, 1:] = [2 * imw, 2 * imh, 2 * imw + 40, 2 * imh + 40]
    r[1, 1:] = [12.0, 20.0, 12.0, 20.0]
    r[2, 1:] = [0, 0, imw - 1, imh - 1]
    return torch.from_numpy(r.astype(np.float32))


_POOL_CACHE = {}


def _pool_case(drn, dtype, C, H, W, R):
    """inputs of one RoIPool backward, computed once per (dtype, shape) and shared (never modified)"""
    key = (dtype, C, H, W, R)
    if key not in _POOL_CACHE:
        feat = _rnd((N_IMG, C, H, W), 21)
        rois = _rois(R, H, W, 22)
        obj = torch.from_numpy(np.random.RandomState(24).rand(R).astype(np.float32))
        fd = feat.permute(0, 2, 3, 1).contiguous().to(DEV).to(dtype)
        out, arg = drn.roi_pool_nhwc(fd, rois.to(DEV), obj.to(DEV), P, SCALE, want_argmax=True)
        g = _q(_rnd((R, C, P, P), 23), dtype)  # the gradient as the device holds it
        gd = torch.zeros_like(out)
        gd[:, : C * P * P] = g.reshape(R, -1).to(DEV).to(dtype)
        _POOL_CACHE[key] = dict(rois=rois, obj=obj, arg=arg, g=g, gd=gd, rois_d=rois.to(DEV), obj_d=obj.to(DEV))
    return _POOL_CACHE[key]


def _align_case(drn, dtype, C, H, W, R, aligned):
    rois = _rois(R, H, W, 25)
    if aligned:
        rois = torch.cat([rois[:1], rois[2:]])  # aligned=True: the degenerate row is dropped, as in test_ops_gpu.py
    R = rois.shape[0]
    g = _q(_rnd((R, C, P, P), 26), dtype)
    gd = torch.zeros((R, drn.kpad(C * P * P, dtype)), dtype=dtype, device=DEV)
    gd[:, : C * P * P] = g.reshape(R, -1).to(DEV).to(dtype)
    return rois, g, gd


def _bits_equal(a, b):
    """bit for bit (torch.equal would let -0.0 pass for +0.0)"""
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


# ----------------------------------------------------------------------------------------- 1. RoIPool == oracle, bit for bit
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("C,H,W,R", CASES)
def test_roi_pool_backward_det_bit_equal_to_oracle(drn, dtype, C, H, W, R):
    """the deterministic RoIPool backward adds in the order of the oracle's sequential scatter (m, then c, then bin; per element
    that is (m, bin)): equal bits, with the objectness scaling folded in as fl32(g * (obj + 1))"""
    k = _pool_case(drn, dtype, C, H, W, R)
    arg_h = k["arg"].cpu().reshape(R, C, P, P)
    assert int((arg_h[0] >= 0).sum()) == 0  # the ROI outside the map: empty bins
    ref = O.roi_pool_backward(k["g"] * (k["obj"] + 1).view(-1, 1, 1, 1), k["rois"], arg_h, (N_IMG, C, H, W))
    d = drn.roi_pool_backward_nhwc(k["gd"], k["rois_d"], k["obj_d"], (N_IMG, H, W, C), P, SCALE, argmax=k["arg"], deterministic=True)
    got = d.permute(0, 3, 1, 2).cpu()
    print("roi_pool det vs oracle: max|diff| = %.3e, max|ref| = %.3e" % (float((got - ref).abs().max()), float(ref.abs().max())))
    assert torch.equal(got, ref)
    assert float(ref.abs().max()) > 0


@pytest.mark.parametrize("dtype", DTYPES)
def test_roi_pool_backward_det_without_objectness(drn, dtype):
    C, H, W, R = CASES[0]
    k = _pool_case(drn, dtype, C, H, W, R)
    ref = O.roi_pool_backward(k["g"], k["rois"], k["arg"].cpu().reshape(R, C, P, P), (N_IMG, C, H, W))
    d = drn.roi_pool_backward_nhwc(k["gd"], k["rois_d"], None, (N_IMG, H, W, C), P, SCALE, argmax=k["arg"], deterministic=True)
    assert torch.equal(d.permute(0, 3, 1, 2).cpu(), ref)
    assert float(ref.abs().max()) > 0


# ----------------------------------------------------------------------------------------- 2. ROIAlign vs the oracle
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("aligned,sr", [(False, 0), (True, 0), (True, 2)])
@pytest.mark.parametrize("C,H,W,R", [(70, 19, 23, 50), (130, 41, 67, 40)])
def test_roi_align_backward_det_vs_oracle(drn, dtype, aligned, sr, C, H, W, R):
    """the project's bound for this op (test_ops_gpu.py: 2e-5 of the largest reference value).  No bit-equality: the oracle
    follows ROIAlign_cpu.cpp's pre-computed weights, and its coordinate arithmetic is not pinned to the device's."""
    rois, g, gd = _align_case(drn, dtype, C, H, W, R, aligned)
    ref = O.roi_align_backward(g, rois, (N_IMG, C, H, W), P, SCALE, sr, aligned)
    d = drn.roi_pool_backward_nhwc(gd, rois.to(DEV), None, (N_IMG, H, W, C), P, SCALE, mode=1, sampling_ratio=sr, aligned=aligned,
                                   deterministic=True)
    got = d.permute(0, 3, 1, 2).cpu()
    err, mag = float((got - ref).abs().max()), float(ref.abs().max())
    print("roi_align det vs oracle: max|diff| = %.3e, max|ref| = %.3e" % (err, mag))
    assert mag > 0
    assert err <= 2e-5 * mag


# ----------------------------------------------------------------------------------------- 3. order properties
def _mode_call(drn, mode, dtype, C, H, W, R):
    """-> (call(gd, rois_d, obj_d, arg, n, c, **kw), gd, rois (host), rois_d, obj_d, arg) for one mode on one shape"""
    if mode == 0:
        k = _pool_case(drn, dtype, C, H, W, R)
        gd, rois, obj_d, arg, ka = k["gd"], k["rois"], k["obj_d"], k["arg"], {}
    else:
        rois, _, gd = _align_case(drn, dtype, C, H, W, R, True)
        obj_d = torch.from_numpy(np.random.RandomState(27).rand(rois.shape[0]).astype(np.float32)).to(DEV)
        arg, ka = None, dict(mode=1, sampling_ratio=2, aligned=True)

    def call(gd, rois_d, obj_d, arg, n, c, **kw):
        return drn.roi_pool_backward_nhwc(gd, rois_d, obj_d, (n, H, W, c), P, SCALE, argmax=arg, deterministic=True, **ka, **kw)

    return call, gd, rois, rois.to(DEV), obj_d, arg


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("C,H,W,R", [(70, 19, 23, 60), (130, 41, 67, 40)])
def test_order_properties(drn, dtype, mode, C, H, W, R):
    call, gd, rois, rois_d, obj_d, arg = _mode_call(drn, mode, dtype, C, H, W, R)
    R = rois.shape[0]
    full = call(gd, rois_d, obj_d, arg, N_IMG, C)
    assert float(full.abs().max()) > 0
    # (a) run to run
    for _ in range(2):
        assert _bits_equal(call(gd, rois_d, obj_d, arg, N_IMG, C), full)
    # (b) per image: image b's ROIs alone, in their original relative order, as image 0 of a batch of one
    for b in range(N_IMG):
        sel = torch.nonzero(rois[:, 0] == b).flatten().to(DEV)
        assert 0 < sel.numel() < R
        r1 = rois_d[sel].clone()
        r1[:, 0] = 0
        one = call(gd[sel].contiguous(), r1, obj_d[sel].contiguous(), None if arg is None else arg[sel].contiguous(), 1, C)
        assert _bits_equal(one[0], full[b]), b
    # (c) per channel: the first 64 channels alone (another chunking of the channels, the same order per element)
    c1 = 64
    g1 = gd[:, : c1 * P * P].contiguous()
    a1 = None if arg is None else arg.reshape(R, C, P * P)[:, :c1].reshape(R, -1).contiguous()
    part = call(g1, rois_d, obj_d, a1, N_IMG, c1)
    assert _bits_equal(part, full[..., :c1])


@pytest.mark.parametrize("mode", [0, 1])
def test_untouched_elements_and_no_rois(drn, mode):
    """(d) every element is stored, zeros included: M == 0 and the unreached part of a map both come out as +0.0 over a buffer
    that held NaN"""
    C, H, W = 70, 19, 23
    ka = dict(mode=1, sampling_ratio=2, aligned=True) if mode else {}
    out = torch.full((N_IMG, H, W, C), float("nan"), device=DEV)
    empty_g = torch.zeros((0, drn.kpad(C * P * P, torch.float32)), device=DEV)
    empty_a = torch.zeros((0, C * P * P), dtype=torch.int32, device=DEV) if mode == 0 else None
    d = drn.roi_pool_backward_nhwc(empty_g, torch.zeros((0, 5), device=DEV), None, (N_IMG, H, W, C), P, SCALE, argmax=empty_a,
                                   deterministic=True, out=out, **ka)
    assert d is out and int(torch.count_nonzero(out.view(torch.int32))) == 0
    # one small ROI in image 1's top-left corner: image 0 and the rest of image 1 stay +0.0
    rois = torch.tensor([[1, 8.0, 8.0, 40.0, 40.0]], device=DEV)
    feat = _rnd((N_IMG, H, W, C), 31).to(DEV)
    arg = drn.roi_pool_nhwc(feat, rois, None, P, SCALE, want_argmax=True)[1] if mode == 0 else None
    g = torch.zeros((1, drn.kpad(C * P * P, torch.float32)), device=DEV)
    g[:, : C * P * P] = _rnd((1, C * P * P), 32).abs().to(DEV) + 0.5
    out.fill_(float("nan"))
    drn.roi_pool_backward_nhwc(g, rois, None, (N_IMG, H, W, C), P, SCALE, argmax=arg, deterministic=True, out=out, **ka)
    assert bool(torch.isfinite(out).all())
    assert int(torch.count_nonzero(out[0].view(torch.int32))) == 0
    assert int(torch.count_nonzero(out[1, 8:].view(torch.int32))) == 0 and int(torch.count_nonzero(out[1, :, 8:].view(torch.int32))) == 0
    assert float(out[1, :7, :7].abs().max()) > 0


# ----------------------------------------------------------------------------------------- 4. capture
@pytest.mark.parametrize("mode", [0, 1])
def test_capturable(drn, mode):
    """the op alone in a graph (its workspace and output come from the graph's pool): each replay equals the eager call"""
    C, H, W, R = CASES[0]
    call, gd, rois, rois_d, obj_d, arg = _mode_call(drn, mode, torch.float32, C, H, W, R)
    static_g = gd.clone()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        call(static_g, rois_d, obj_d, arg, N_IMG, C)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        static_d = call(static_g, rois_d, obj_d, arg, N_IMG, C)
    for data in (gd, gd.flip(0) * 0.5 + 1.0):
        static_g.copy_(data)
        graph.replay()
        torch.cuda.synchronize()
        assert _bits_equal(static_d, call(data.contiguous(), rois_d, obj_d, arg, N_IMG, C))


# ----------------------------------------------------------------------------------------- 5. whole model, run to run
def _forever(batch):
    while True:
        yield batch


def _params(model):
    return {n: p.detach().clone() for n, p in model.named_parameters() if p.requires_grad}


def test_csc_training_repeats_bit_for_bit():
    """set_deterministic(True): the tiny CSC model (csc_WSR_18_DC5_1x.yaml scaled down; its image-gradient passes run the RoIPool
    backward) trained twice from scratch for three steps on one batch - every loss of every step and every trainable parameter
    afterwards bit-identical; the first run stays within the reference bound of test_csc_model_three_steps_vs_reference."""
    from drn_wsod_pytorch_amd.engine import build_optimizer

    pkg = load_package()
    assert pkg.get_deterministic() is False
    pkg.set_deterministic(True)
    try:
        runs = []
        for _ in range(2):
            ocfg = G.csc_case()
            d = G.load("model_csc_r18dc5_tiny")
            cfg, model = G.drn_model(ocfg, int(d["seed"]), DEV, 5, "fp32")
            model.roi_heads.box_head.dropout_p = 0.0
            model.roi_heads.tau = float(d["tau"])
            model.roi_heads.iter = int(d["iter0"])
            model.train()
            assert model.cpg and model.backbone.input_grad
            opt = build_optimizer(cfg, model)
            batch = G.drn_inputs(G.batch_from(d))
            losses = []
            for step in range(3):
                opt.zero_grad()
                ld = model(batch)
                sum(ld.values()).backward()
                losses.append({k: v.detach().clone() for k, v in ld.items()})
                opt.step()
            torch.cuda.synchronize()
            runs.append((losses, _params(model)))
            if len(runs) == 1:
                for step, ld in enumerate(losses):
                    for k, v in ld.items():
                        ref = float(d["step%d_%s" % (step, k)])
                        assert abs(float(v) - ref) <= 2e-4 * max(1.0, abs(ref)) + 1e-9, (step, k, float(v), ref)
            del model, opt
        (l0, p0), (l1, p1) = runs
        for step in range(3):
            assert sorted(l0[step]) == sorted(l1[step])
            for k in l0[step]:
                assert _bits_equal(l0[step][k].reshape(1).float(), l1[step][k].reshape(1).float()), (step, k)
        assert sorted(p0) == sorted(p1) and p0
        for n in p0:
            assert torch.equal(p0[n], p1[n]), n
    finally:
        pkg.set_deterministic(False)


def test_trainable_trunk_training_repeats_bit_for_bit():
    """set_deterministic(True): the tiny R50-C4 OICR model with FREEZE_AT = 3 (fc6 dX -> RoIPool backward -> trunk backward),
    two steps of the eager Trainer, twice from scratch: losses and every trainable parameter bit-identical"""
    from drn_wsod_pytorch_amd.engine import Trainer, build_optimizer

    pkg = load_package()
    pkg.set_deterministic(True)
    try:
        runs = []
        for _ in range(2):
            name = "model_r50c4_tiny"
            ocfg, d = G.MODEL_CASES[name], G.load(name)
            cfg, model = G.drn_model(ocfg, int(d["seed"]), DEV, 3, "fp32")
            model.roi_heads.box_head.dropout_p = 0.0
            model.train()
            assert any(n.startswith("backbone.") for n, p in model.named_parameters() if p.requires_grad)
            tr = Trainer(cfg, model, _forever(G.drn_inputs(G.batch_from(d))), optimizer=build_optimizer(cfg, model))
            losses = []
            for _step in range(2):
                losses.append({k: v.detach().clone() for k, v in tr.run_step().items()})
            torch.cuda.synchronize()
            runs.append((losses, _params(model)))
            del model, tr
        (l0, p0), (l1, p1) = runs
        for step in range(2):
            for k in l0[step]:
                assert bool(torch.isfinite(l0[step][k]))
                assert _bits_equal(l0[step][k].reshape(1).float(), l1[step][k].reshape(1).float()), (step, k)
        assert sorted(p0) == sorted(p1) and p0
        for n in p0:
            assert torch.equal(p0[n], p1[n]), n
    finally:
        pkg.set_deterministic(False)
        pkg.set_precision("fp32")
