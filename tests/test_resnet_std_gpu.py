"""GPU tests of the plain-ResNet WSDDN recipes (wsddn_R_50_DC5_1x.yaml, wsddn_R_101_DC5_1x.yaml): the 3x3 / stride-2 / pad-1 max
pool against torch bit for bit, the stem's 7x7 / stride-2 conv and the trunk's stride-2 1x1 convs against F.conv2d under the
bounds of tests/test_ops_gpu.py, the trunk's launch plan against its per-layer walk bit for bit, and both whole models against
the goldens of the unmodified reference (tests/golden/gen_golden_resnet.py) under the tolerances of tests/test_model_gpu.py -
fp32 parity mode and bf16 - plus a captured training step against the eager pipelined one."""
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import golden_util as G
import resnet_std_util as U
from __graft_entry__ import load_package

pytestmark = pytest.mark.gpu
O = G.O
DEV = "cuda"
DTYPES = [torch.float32, torch.bfloat16]


@pytest.fixture(scope="module")
def drn():
    assert torch.cuda.is_available(), "GPU tests need a GPU (run with -m gpu on the MI355X box)"
    pkg = load_package()
    pkg._cabi.lib()
    import importlib

    return importlib.import_module("drn_wsod_pytorch_amd.ops")


@pytest.fixture(autouse=True)
def _fp32_after():
    yield
    load_package().set_precision("fp32")


def _rnd(shape, seed, scale=1.0):
    return torch.from_numpy(np.random.RandomState(seed).standard_normal(shape).astype(np.float32) * scale)


def _q(x, dtype):
    return x.to(dtype).float()


def _relerr(a, b, floor=1e-6):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.abs(a - b).max() / (np.abs(b).max() + floor))


# ------------------------------------------------------------------------------------------------- 5. the 3x3 max pool
POOL_CASES = [(1, 1, 1, 8), (1, 1, 5, 8), (1, 6, 1, 16), (2, 2, 2, 16), (1, 2, 3, 8), (1, 3, 3, 64), (1, 7, 9, 64), (3, 13, 6, 24),
              (1, 112, 112, 64), (1, 400, 608, 64), (1, 401, 607, 64), (2, 57, 608, 72), (2, 608, 3, 8)]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("sign", ["mixed", "negative"])
@pytest.mark.parametrize("case", POOL_CASES)
def test_maxpool3x3s2_equals_torch(drn, dtype, sign, case):
    n, h, w, c = case
    x = _rnd((n, c, h, w), 91 + h + w)
    if sign == "negative":  # zero or any finite padding value would win somewhere along the border
        x = -x.abs() - 1.0
    xq = _q(x, dtype)
    ref = F.max_pool2d(xq, kernel_size=3, stride=2, padding=1)
    y = drn.maxpool3x3s2_nhwc(xq.permute(0, 2, 3, 1).contiguous().to(DEV).to(dtype))
    assert y.dtype == dtype and tuple(y.shape) == (n, (h + 2 - 3) // 2 + 1, (w + 2 - 3) // 2 + 1, c)
    assert torch.equal(y.float().cpu().permute(0, 3, 1, 2), ref)


def test_maxpool3x3s2_fp8_nonnegative(drn):
    """the quantised trunk's pool: e4m3 bytes of non-negative values order like the values"""
    x = _rnd((2, 32, 37, 41), 5).abs().clamp(max=400.0)
    xq = x.to(drn.FP8)
    y = drn.maxpool3x3s2_nhwc(xq.permute(0, 2, 3, 1).contiguous().to(DEV))
    ref = F.max_pool2d(xq.float(), 3, 2, 1)
    assert y.dtype == drn.FP8 and torch.equal(y.float().cpu().permute(0, 3, 1, 2), ref)


# ------------------------------------------------------------------ 6. the stem conv and the stride-2 1x1 convs of the trunk
def _padded(x2d, dtype, drn):
    r, k = x2d.shape
    out = torch.zeros((r, drn.kpad(k, dtype)), dtype=dtype, device=DEV)
    out[:, :k] = x2d.to(DEV).to(dtype)
    return out


def _pack_w(w, dtype, drn, cin_pad):
    cout, cin, kh, kw = w.shape
    wp = torch.zeros((cout, kh, kw, cin_pad))
    wp[..., :cin] = w.permute(0, 2, 3, 1)
    return _padded(wp.reshape(cout, -1), dtype, drn)


STRIDED_CASES = [
    # (N, H, W, Cin, Cout, k, stride, pad, dil, residual, relu)
    (1, 224, 224, 3, 64, 7, 2, 3, 1, False, True),      # BasicStem.conv1 (resnet.py:344-352)
    (2, 97, 131, 3, 64, 7, 2, 3, 1, False, True),       # odd sizes, two images
    (1, 800, 1216, 3, 64, 7, 2, 3, 1, False, True),     # the recipe's training size
    (1, 23, 9, 3, 64, 7, 2, 3, 1, False, False),
    (1, 56, 56, 256, 128, 1, 2, 0, 1, False, True),     # res3.0.conv1 (STRIDE_IN_1X1) at 224 x 224
    (1, 56, 56, 256, 512, 1, 2, 0, 1, False, False),    # res3.0.shortcut
    (1, 28, 28, 512, 256, 1, 2, 0, 1, False, True),     # res4.0.conv1
    (1, 28, 28, 512, 1024, 1, 2, 0, 1, False, False),   # res4.0.shortcut
    (1, 14, 14, 1024, 512, 1, 2, 0, 1, False, True),    # res5.0.conv1 (RES5_DILATION 1)
    (1, 14, 14, 1024, 2048, 1, 2, 0, 1, False, False),  # res5.0.shortcut
    (1, 200, 304, 256, 128, 1, 2, 0, 1, False, True),   # the same layers at 800 x 1216
    (1, 200, 304, 256, 512, 1, 2, 0, 1, False, False),
    (1, 100, 152, 512, 256, 1, 2, 0, 1, False, True),
    (1, 100, 152, 512, 1024, 1, 2, 0, 1, False, False),
    (1, 50, 76, 1024, 512, 1, 2, 0, 1, False, True),
    (1, 50, 76, 1024, 2048, 1, 2, 0, 1, False, False),
    (2, 57, 75, 256, 512, 1, 2, 0, 1, True, True),      # odd map, two images, a residual behind the strided conv
    (1, 28, 28, 512, 1024, 1, 2, 0, 1, True, True),
    (1, 13, 14, 1024, 2048, 1, 2, 0, 1, True, False),
]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("case", STRIDED_CASES)
def test_strided_trunk_convs(drn, dtype, case):
    n, h, w, cin, cout, k, stride, pad, dil, has_res, relu = case
    x = _rnd((n, cin, h, w), 5)
    wt = _rnd((cout, cin, k, k), 6, math.sqrt(2.0 / (cin * k * k)))
    scale, bias = 0.8 + 0.2 * torch.rand(cout), _rnd((cout,), 7, 0.1)
    cin_pad = (8 if dtype == torch.bfloat16 else 4) if cin == 3 else cin
    xd = torch.zeros((n, h, w, cin_pad), dtype=dtype, device=DEV)
    xd[..., :cin] = x.permute(0, 2, 3, 1).to(DEV).to(dtype)
    ref = F.conv2d(_q(x, dtype), _q(wt, dtype), None, stride, pad, dil) * scale.view(1, -1, 1, 1) + bias.view(1, -1, 1, 1)
    res = None
    if has_res:
        res = _rnd(tuple(ref.shape), 8)
        ref = ref + _q(res, dtype)
        res = res.permute(0, 2, 3, 1).contiguous().to(DEV).to(dtype)
    if relu:
        ref = F.relu(ref)
    y = drn.conv2d_nhwc(xd, _pack_w(wt, dtype, drn, cin_pad), cout, k, k, stride, pad, dil, scale.to(DEV), bias.to(DEV), res, relu)
    got = y.float().cpu().permute(0, 3, 1, 2)
    assert got.shape == ref.shape
    err = float((got - ref).abs().max())
    print("strided conv", case, dtype, "max abs err %.3e" % err)
    if dtype == torch.float32:  # the bounds of tests/test_ops_gpu.py::test_conv2d_nhwc / test_pp8_conv_kernel
        assert torch.allclose(got, ref, rtol=1e-4, atol=1e-4), err
    else:
        assert torch.allclose(got, ref, rtol=2 ** -7, atol=2e-2), err


# ------------------------------------------------------------------------- 7. the launch plan against the per-layer walk
def _both(bb, x):
    with torch.no_grad():
        bb.use_plan = True
        a = bb(x)
        bb.use_plan = False
        b = bb(x)
        bb.use_plan = True
    return a, b


def _image_batches(sizes, seed=0):
    rs = np.random.RandomState(seed)
    return [torch.from_numpy((rs.randint(0, 256, (n, 3, h, w)).astype(np.float32) - 110.0)).to(DEV) for n, h, w in sizes]


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
@pytest.mark.parametrize("name", sorted(U.CASES))
def test_plan_equals_per_layer_walk_tiny(name, precision, tmp_path):
    cfg, model, d = U.tiny_model(name, tmp_path, DEV, precision)
    model.eval()
    bb = model.backbone
    for x in _image_batches([(1, 64, 64), (2, 97, 131), (1, 33, 47), (1, 160, 192), (1, 40, 56)]):
        a, b = _both(bb, x)
        assert list(a) == list(b) == ["res5"]
        assert a["res5"].shape == b["res5"].shape and a["res5"].dtype == b["res5"].dtype
        assert torch.equal(a["res5"], b["res5"]), (name, precision, tuple(x.shape))
    p = next(iter(bb._plans.values()))
    assert p["n_slots"] <= 7 and (p["ops"][1].kind & 0xff) == 2


@pytest.mark.parametrize("yaml_rel", [U.R50, U.R101])
def test_plan_equals_per_layer_walk_full_width(yaml_rel, tmp_path):
    """the two trunks at full width, bf16, at 800 x 1216, two ragged-size images and 224 x 224: the plan (res2's 3x3 + 1x1 pairs as
    one launch on the large maps, everything else one launch per layer) and the per-layer walk give the same bits; the map has
    the recipe's stride and is not degenerate"""
    from drn_wsod_pytorch_amd.modeling import build_backbone

    load_package().set_precision("bf16")
    bb = build_backbone(U.recorded_cfg(yaml_rel, tmp_path, device=DEV)).to(DEV).eval()
    bb.load_state_dict({n: O.seeded_tensor("backbone." + n, tuple(t.shape), 3) for n, t in bb.state_dict().items()})
    stride = 32 if yaml_rel == U.R50 else 16
    for x in _image_batches([(1, 800, 1216), (2, 601, 799), (1, 224, 224)], seed=3):
        a, b = _both(bb, x)
        f = a["res5"]
        hs = [(s - 1) // 2 + 1 for s in x.shape[2:]]            # conv 7x7 / 2 / 3
        hs = [(s - 1) // 2 + 1 for s in hs]                        # pool 3x3 / 2 / 1
        for _ in range({32: 3, 16: 2}[stride]):
            hs = [(s - 1) // 2 + 1 for s in hs]                    # 1x1 / 2
        assert tuple(f.shape) == (x.shape[0], 2048, hs[0], hs[1])
        assert torch.equal(f, b["res5"]), (yaml_rel, tuple(x.shape))
        assert torch.isfinite(f.float()).all() and float(f.float().abs().max()) > 0
    p = next(iter(bb._plans.values()))
    assert sum(1 for i in range(p["n_ops"]) if p["ops"][i].kind & 0x100) == 3  # res2: conv2 + conv3 pairs
    assert not any(p["ops"][i].kind & 0x200 for i in range(p["n_ops"]))        # the 2x2-pool epilogue is not for this stem
    assert p["ops"][0].kind & 0x400 and (p["ops"][1].kind & 0xff) == 2            # the stem pair: one launch in the plan


FUSED_STEM_SIZES = [(1, 1, 1), (1, 2, 3), (1, 7, 9), (1, 23, 40), (1, 33, 31), (2, 57, 75), (1, 97, 131), (1, 224, 224), (3, 64, 48),
                    (2, 601, 799), (1, 800, 1216), (1, 801, 1215)]


@pytest.mark.parametrize("size", FUSED_STEM_SIZES)
def test_fused_stem_equals_conv_then_pool(drn, size):
    """drn_stem7x7_pool_nhwc == drn_conv2d_nhwc + drn_maxpool3x3s2_nhwc, bit for bit: tiny, odd, 224 x 224, 800 x 1216, batches;
    mixed-sign affine so that ReLU zeroes a good part of the conv map (the pool then meets runs of equal values)"""
    n, h, w = size
    dtype = torch.bfloat16
    x = _rnd((n, 3, h, w), 31 + h, 60.0)
    wt = _rnd((64, 3, 7, 7), 32, math.sqrt(2.0 / (3 * 49)))
    scale, bias = (0.8 + 0.2 * torch.rand(64)).to(DEV), _rnd((64,), 33, 20.0).to(DEV)
    xd = torch.zeros((n, h, w, 8), dtype=dtype, device=DEV)
    xd[..., :3] = x.permute(0, 2, 3, 1).to(DEV).to(dtype)
    wp = _pack_w(wt, dtype, drn, 8)
    conv = drn.conv2d_nhwc(xd, wp, 64, 7, 7, 2, 3, 1, scale, bias, None, True)
    two = drn.maxpool3x3s2_nhwc(conv)
    one = drn.stem7x7_pool_nhwc(xd, wp, 64, scale, bias, True)
    assert one is not None, "inside the kernel's class"
    torch.cuda.synchronize()
    assert one.shape == two.shape and one.dtype == two.dtype
    frac_zero = float((two == 0).float().mean())
    ndiff = int((one != two).sum())
    print("fused stem", size, "pooled", tuple(two.shape), "zeros %.2f" % frac_zero, "differing elements", ndiff)
    assert torch.equal(one, two), (size, ndiff)
    assert float(two.float().abs().max()) > 0
    # against the definition as well (CPU, rounded operands), under the conv tests' bf16 bound
    ref = F.max_pool2d(F.relu(F.conv2d(_q(x, dtype), _q(wt, dtype), None, 2, 3) * scale.cpu().view(1, -1, 1, 1)
                              + bias.cpu().view(1, -1, 1, 1)), 3, 2, 1)
    got = one.float().cpu().permute(0, 3, 1, 2)
    assert torch.allclose(got, ref, rtol=2 ** -7, atol=2e-2), float((got - ref).abs().max())


def test_fused_stem_refuses_outside_its_class(drn):
    """fp32, other channel counts, no ReLU: DRN_ERR_UNSUPPORTED (the wrapper's None) - the callers run the two launches, which is
    what the fp32 plan and the narrow tiny trunks do (their plans carry no flag, see the plan tests)"""
    for dtype, cin, cout, relu in [(torch.float32, 4, 64, True), (torch.bfloat16, 8, 32, True), (torch.bfloat16, 16, 64, True),
                                   (torch.bfloat16, 8, 64, False)]:
        xd = torch.zeros((1, 32, 32, cin), dtype=dtype, device=DEV)
        wp = torch.zeros((cout, drn.kpad(49 * cin, dtype)), dtype=dtype, device=DEV)
        sc, bi = torch.ones(cout, device=DEV), torch.zeros(cout, device=DEV)
        assert drn.stem7x7_pool_nhwc(xd, wp, cout, sc, bi, relu) is None, (dtype, cin, cout, relu)
        y = drn.maxpool3x3s2_nhwc(drn.conv2d_nhwc(xd, wp, cout, 7, 7, 2, 3, 1, sc, bi, None, relu))  # the two launches take it
        assert tuple(y.shape) == (1, 8, 8, cout)


# ---------------------------------------------------------------------------- 8. whole models, fp32 parity mode, goldens
def _prep(model, d):
    masks = G.dropmasks_from(d)
    assert masks is None
    model.roi_heads.box_head.dropout_p = 0.0  # fixtures were generated with dropout patched to identity
    return G.batch_from(d)


@pytest.mark.parametrize("name", sorted(U.CASES))
def test_two_steps_and_inference_fp32(name, tmp_path):
    from drn_wsod_pytorch_amd.engine import build_optimizer

    cfg, model, d = U.tiny_model(name, tmp_path, DEV, "fp32")
    base = _prep(model, d)
    # the trunk's map first (frozen: the fixture's map, taken after the two steps, is the one of the initial weights)
    model.eval()
    with torch.no_grad():
        images = model.preprocess_image(G.drn_inputs(base, False))
        feats = model.backbone(images.tensor)
    f = feats[str(d["feat_name"])].float().cpu().numpy()
    assert f.shape == d["feat"].shape and f.shape[2] >= 5 and f.shape[3] >= 6
    e = _relerr(f, d["feat"])
    print(name, "res5 rel err %.3e, max |res5| %.3f" % (e, float(np.abs(d["feat"]).max())))
    assert e < 1e-4
    batch = G.drn_inputs(base)
    model.train()
    opt = build_optimizer(cfg, model)
    before = {n: p.detach().clone() for n, p in model.named_parameters() if p.requires_grad}
    assert sorted(before) == sorted(d["trainable"].tolist())
    for step in range(2):
        opt.zero_grad()
        losses = model(batch)
        assert sorted(losses) == ["loss_cls"]
        sum(losses.values()).backward()
        for k, v in losses.items():
            v, ref = float(v.detach()), float(d["step%d_%s" % (step, k)])
            print(name, "step", step, k, v, ref, "rel %.3e" % (abs(v - ref) / max(abs(ref), 1e-3)))
            assert abs(v - ref) <= 1e-4 * max(abs(ref), 1e-3), (step, k, v, ref)
        if step == 0:
            for n, p in model.named_parameters():
                if not p.requires_grad:
                    continue
                g = p.grad.detach().cpu().numpy()
                if "grad0." + n in d:
                    ref_g = d["grad0." + n]
                    if np.abs(ref_g).max() < 1e-6:  # analytically zero (det bias): both sides are rounding noise
                        assert np.abs(g).max() < 1e-5, n
                    else:
                        assert _relerr(g, ref_g) < 2e-3, (n, _relerr(g, ref_g))
                else:
                    assert _relerr(g.reshape(-1)[:4096], d["gradhead0." + n]) < 2e-3, n
                    ref_abs = float(d["gradabs0." + n])
                    assert abs(float(np.abs(g.astype(np.float64)).sum()) - ref_abs) < 2e-3 * ref_abs, n
        opt.step()
        if step == 0:
            for n, p in model.named_parameters():
                if p.requires_grad and p.grad is not None:
                    lr = cfg.SOLVER.BASE_LR * (2.0 if n.endswith("bias") else 1.0)
                    wd = 0.0 if n.endswith("bias") else cfg.SOLVER.WEIGHT_DECAY
                    exp = before[n] - lr * (p.grad + wd * before[n])
                    assert torch.allclose(p.detach(), exp, rtol=1e-5, atol=1e-7), n
    for n, p in model.named_parameters():
        if p.requires_grad:
            got = p.detach().reshape(-1)[:2048].cpu().numpy()
            assert _relerr(got, d["after2.head." + n]) < 5e-3, (n, _relerr(got, d["after2.head." + n]))
    # inference with the updated weights: the fixture's scores and detections
    model.eval()
    with torch.no_grad():
        res, all_scores, all_boxes = model.inference(G.drn_inputs(base, False), do_postprocess=False)
        out = model(G.drn_inputs(base, False))
    assert len(out) == len(base) and "instances" in out[0]
    for i in range(len(base)):
        ref_s = d["all_scores%d" % i]
        got_s = all_scores[i].float().cpu().numpy().reshape(ref_s.shape)
        print(name, "image", i, "all_scores rel err %.3e" % _relerr(got_s, ref_s), "detections", len(res[i]), len(d["det%d_scores" % i]))
        assert _relerr(got_s, ref_s) < 1e-4
        assert len(res[i]) == len(d["det%d_scores" % i])
        assert torch.equal(res[i].pred_classes.cpu(), torch.from_numpy(d["det%d_classes" % i]))
        # WSDDN does not regress: a detection's box IS its proposal, so equal boxes are equal kept indices
        assert torch.equal(res[i].pred_boxes.tensor.cpu(), torch.from_numpy(d["det%d_boxes" % i]))
        assert torch.allclose(res[i].scores.cpu(), torch.from_numpy(d["det%d_scores" % i]), rtol=1e-3, atol=1e-6)


# --------------------------------------------------------------------------------------------------------- 9. bf16 mode
@pytest.mark.parametrize("name", sorted(U.CASES))
def test_train_step_bf16(name, tmp_path):
    """bf16 fast mode on the same fixtures: loss agreement within 3e-2 relative (tests/test_model_gpu.py::test_train_step_bf16),
    finite gradients"""
    cfg, model, d = U.tiny_model(name, tmp_path, DEV, "bf16")
    batch = G.drn_inputs(_prep(model, d))
    model.train()
    losses = model(batch)
    sum(losses.values()).backward()
    for k, v in losses.items():
        ref = float(d["step0_%s" % k])
        print(name, "bf16", k, float(v.detach()), ref)
        assert abs(float(v.detach()) - ref) <= 3e-2 * max(abs(ref), 1e-2), (k, float(v.detach()), ref)
    for n, p in model.named_parameters():
        if p.requires_grad and p.grad is not None:
            assert torch.isfinite(p.grad).all(), n


def _fixed_shape_batches(d, num_classes):
    """three different single-image batches of one shape (a captured step needs static shapes)"""
    base = G.batch_from(d)
    alt = dict(base[0])
    alt["image"] = (255.0 - base[0]["image"]).contiguous()
    alt["objectness_logits"] = base[0]["objectness_logits"].flip(0).contiguous()
    alt2 = dict(base[0])
    alt2["image"] = base[0]["image"].flip(2).contiguous()
    alt2["proposal_boxes"] = base[0]["proposal_boxes"].flip(0).contiguous()
    alt2["gt_classes"] = (base[0]["gt_classes"] + 1) % num_classes
    return [G.drn_inputs([b]) for b in (base[0], alt, alt2)]


@pytest.mark.parametrize("fc_dim", [64, 1024])
def test_graphed_step_equals_eager_pipelined_bf16(fc_dim, tmp_path):
    """GraphedTrainStep over the R-50 model (FastRCNNConvFCHead, no dropout) at one fixed shape, bf16, the pipelined optimizer:
    the losses of eight steps over a cycle of three batches that is not periodic are the eager pipelined step's, bit for bit.
    fc_dim 1024 is the recipe's head width (D1 = D2 = 1024 through the head engine's fused launches or their fallbacks) on the
    tiny trunk; 64 is the fixture's."""
    from drn_wsod_pytorch_amd.engine import GraphedTrainStep, build_optimizer
    from drn_wsod_pytorch_amd.modeling import build_model

    name = "model_r50std_tiny"
    d = G.load(name)
    K = 5
    b0, b1, b2 = _fixed_shape_batches(d, K)
    seq = [b0, b1, b2, b0, b1, b1, b0, b2, b1, b0, b2, b2]
    steps = 8
    results = []
    for graphed in (False, True):
        load_package().set_precision("bf16")
        opts = [str(o) for o in d["cfg_opts"]]
        # (the recipe's BASE_LR 0.01 saturates this toy net's BCE within two steps - every later loss is one of two clamped
        # values; at 2e-4 the losses keep moving, so a stale weight or a wrong slot shows at any step)
        cfg = U.recorded_cfg(opts[0], tmp_path, opts[1:] + ["MODEL.ROI_BOX_HEAD.FC_DIM", str(fc_dim), "SOLVER.BASE_LR", "0.0002"],
                             DEV)
        model = build_model(cfg)
        sd = model.state_dict()
        model.load_state_dict({n: (t if n in ("pixel_mean", "pixel_std") else O.seeded_tensor(n, tuple(t.shape), 71))
                               for n, t in sd.items()})
        assert type(model.roi_heads.box_head).__name__ == "FastRCNNConvFCHead" and model.roi_heads.box_head.dropout_p == 0.0
        assert tuple(model.roi_heads.box_head.fc2.weight.shape) == (fc_dim, fc_dim)
        model.train()
        opt = build_optimizer(cfg, model)
        opt.enable_pipelined()
        out = []
        if graphed:
            stepper = GraphedTrainStep(model, opt, seq[0], split_tail=True, eager_fc6=True)
            for i in range(steps):
                losses = stepper.step(*seq[i: i + 3])
                out.append({k: float(v.detach()) for k, v in losses.items()})
            stepper.release()
        else:
            for i in range(steps):
                losses = model(seq[i])
                sum(losses.values()).backward()
                opt.step()
                opt.zero_grad()
                out.append({k: float(v.detach()) for k, v in losses.items()})
        torch.cuda.synchronize()
        results.append(out)
        del model, opt
        torch.cuda.empty_cache()
    for i, (e, g) in enumerate(zip(*results)):
        print("fc_dim", fc_dim, "step", i, e, g)
    for i, (e, g) in enumerate(zip(*results)):
        assert sorted(e) == sorted(g) == ["loss_cls"]
        assert math.isfinite(e["loss_cls"]) and e["loss_cls"] == g["loss_cls"], (i, e, g)
    assert len({r["loss_cls"] for r in results[0]}) > steps // 2  # the weights move and the batches differ: the losses keep changing
