"""The trunk's explicit backward against float64, element by element, at tile edges and layer by layer.

What runs here (references, bounds and case tables: trunk_bwd_util.py; their own checks: test_trunk_bwd_cpu.py):
  1. the pool.hip kernels on their own: im2col_t (bit-exact, padding columns and everything outside a caller's `out` untouched),
     maxpool2x2_bwd_nhwc (stride 2 bit-exact, stride 1 within 3 eps32 sum|dy|, ties and all-zero windows planted), add (bit-exact);
  2. Conv2d.backward_nhwc, one layer, every argument: relu / residual (d_res bit-exact), FrozenBN scale and the VGG bias form,
     need_dx True for every stride and False (None), accumulate False on garbage then True, dx_only (no gradient tensor changes),
     dy in the compute dtype and in fp32 - dW and dx per element inside 4 eps32 sqrt(L) mag + 1e-6 (+ the storage terms);
     and _dgrad through every forward kernel the trainable trunks' dgrad convs reach (table below), each on the smallest map that
     still plans to that kernel;
  3. BasicStem / BasicBlock / BottleneckBlock / PlainBlock.backward_nhwc against a float64 chain written layer by layer from the
     tensors the device saved, with the tolerance measured by a storage emulation of the same chain (device error <= 4 x the
     emulation's + 1e-6, as relative L2 and as max-abs over tensor-max).

ReLU masks and pool routing always come from the device's own saved forward tensors; the forward is checked separately (the
saved mask may differ from the float64 mask only inside the forward bound, and on at most 0.1 % of the outputs).

The dgrad convs (conv2d_nhwc(g, packed_dgrad, cin_pad, k, k, 1, d(k-1) - p, d)) of the trainable units at the bench image size
(1 x 224 x 224), as the host-only ops.conv2d_plan lists them on a 256-CU device with the default knobs:

    trunk    FREEZE_AT  dtype  forward kernels serving the dgrad convs
    r50c4    2          bf16   KS, TILED_64
    r50c4    2          fp32   KS, TILED_64
    r18dc5   1          bf16   K2, KS, TILED_64
    r18dc5   1          fp32   K2, KS, TILED_64
    vgg16    0          bf16   K2, KS, PATCH_C64, RING_64
    vgg16    0          fp32   K2, KS, TILED_128X64, TILED_64

(test_trunk_bwd_cpu.py::test_dgrad_kind_table re-derives the table and the "smallest map" of every pinned case.)

Measured on an MI355X when these tests were written (worst error / bound over all cases of a check; 1 is the bound):

    im2col_t, add, maxpool2x2_bwd stride 2, d_res, dx_only                  bit-exact
    maxpool2x2_bwd stride 1, fp32                                            0.76
    forward (for the mask check)          fp32 0.13          bf16 0.98 (the bf16 store itself)
    dW, first / accumulated               fp32 0.08 / 0.04   bf16 exact g 0.009 / 0.009   bf16 general 0.32 / 0.25
    dx                                    fp32 0.14          bf16 exact g 0.99 (the store) bf16 general 0.75
    bias gradient (VGG form)              0.00 on the coarse dy grid (the sums are exact in fp32), 0.008 with a general dy
    dgrad by forward kernel               fp32: KS 0.01, K2 0.02, TILED_64 0.06, TILED_128X64 0.06
                                          bf16: K2 0.93, KS 0.95, TILED_64 0.97, RING_64 0.98, PATCH_C64 0.99 (the store)

Block backwards, worst tensor of each case, error against the float64 chain (device must be <= 4 x emulation + 1e-6):

    case                     dtype  L2 device  L2 emul.  max device max emul.
    stem_odd                 fp32   2.72e-07  2.40e-07  3.56e-07  2.37e-07
    stem_odd                 bf16   4.03e-03  4.03e-03  5.01e-03  5.01e-03
    stem_even                fp32   2.54e-07  2.17e-07  4.18e-07  2.29e-07
    stem_even                bf16   4.11e-03  4.10e-03  4.33e-03  4.33e-03
    basic_proj_pool2         fp32   2.86e-07  1.61e-07  5.21e-07  2.27e-07
    basic_proj_pool2         bf16   3.24e-03  3.24e-03  4.76e-03  4.76e-03
    basic_id_nopool_dil2     fp32   2.86e-07  2.43e-07  3.09e-07  2.61e-07
    basic_id_nopool_dil2     bf16   2.92e-03  2.92e-03  2.63e-03  2.63e-03
    basic_id_pool1_dil2      fp32   2.15e-07  1.76e-07  3.50e-07  2.80e-07
    basic_id_pool1_dil2      bf16   3.68e-03  3.68e-03  3.63e-03  3.63e-03
    bottle_proj_pool1_dil2   fp32   2.46e-07  1.98e-07  3.82e-07  2.14e-07
    bottle_proj_pool1_dil2   bf16   4.17e-03  4.17e-03  5.21e-03  5.21e-03
    bottle_id_pool2          fp32   3.85e-07  2.36e-07  4.47e-07  3.04e-07
    bottle_id_pool2          bf16   3.98e-03  3.98e-03  4.70e-03  4.70e-03
    bottle_proj_nopool       fp32   2.72e-07  2.32e-07  3.87e-07  2.31e-07
    bottle_proj_nopool       bf16   4.50e-03  4.50e-03  8.01e-03  8.01e-03
    plain2_pool2             fp32   3.42e-07  2.58e-07  4.48e-07  4.21e-07
    plain2_pool2             bf16   2.41e-03  2.41e-03  3.34e-03  3.34e-03
    plain3_dil2              fp32   3.25e-07  2.94e-07  3.96e-07  3.31e-07
    plain3_dil2              bf16   2.89e-03  2.89e-03  4.23e-03  4.23e-03

(in bf16 the storage rounding dominates both columns, which is why they agree; every assertion message prints its own pair)"""
import importlib
import math

import pytest
import torch

import trunk_bwd_util as U
from __graft_entry__ import load_package

pytestmark = pytest.mark.gpu
DEV = "cuda"


@pytest.fixture(scope="module")
def drn():
    assert torch.cuda.is_available(), "GPU tests need a GPU (run with -m gpu on the MI355X box)"
    pkg = load_package()
    pkg._cabi.lib()  # raises if the HIP library is missing: no fallback
    return importlib.import_module("drn_wsod_pytorch_amd.ops")


def _nhwc_dev(x_nchw, dtype, cpad=None, fill=0.0):
    """[N,C,H,W] cpu -> [N,H,W,Cpad] device tensor of dtype; the channel padding holds `fill`"""
    n, c, h, w = x_nchw.shape
    cp = cpad or c
    out = torch.full((n, h, w, cp), fill, dtype=dtype, device=DEV)
    out[..., :c] = x_nchw.permute(0, 2, 3, 1).to(DEV).to(dtype)
    return out


def _nchw_cpu(t_nhwc, c=None):
    t = t_nhwc.float().cpu().permute(0, 3, 1, 2)
    return t[:, :c] if c is not None else t


def _report(what, ratio):
    print("RATIO %s %.4f" % (what, ratio))
    return ratio


# ---- 1. pool.hip kernels on their own -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", U.DTYPES, ids=U.dname)
@pytest.mark.parametrize("case", U.IM2COL_CASES, ids=str)
def test_im2col_t(drn, case, dtype):
    n, h, w, cin, k, stride, pad, dil = case
    x = U.rnd((n, cin, h, w), 21).to(dtype)
    xd = _nhwc_dev(x, dtype, U.cin_pad(cin, dtype), fill=5.0)  # channel padding never read: it must not show up anywhere
    ref = U.im2col_t_ref(x, k, stride, pad, dil)
    R, P = ref.shape
    Pp = drn.kpad(P, dtype)
    got = drn.im2col_t(xd, cin, k, k, stride, pad, dil).cpu()
    assert got.shape == (R, Pp)
    assert torch.equal(got[:, :P], ref)
    assert (got[:, P:] == 0).all()
    out = torch.full((R + 1, Pp + 64), 7.0, dtype=dtype, device=DEV)
    got = drn.im2col_t(xd, cin, k, k, stride, pad, dil, out=out).cpu()
    assert torch.equal(got[:R, :P], ref)
    assert (got[:R, P:] == 7.0).all() and (got[R:] == 7.0).all()


@pytest.mark.parametrize("dtype", U.DTYPES, ids=U.dname)
@pytest.mark.parametrize("stride", [2, 1])
@pytest.mark.parametrize("shape", U.POOL_BWD_SHAPES, ids=str)
def test_maxpool2x2_bwd(drn, shape, stride, dtype):
    n, h, w, c = shape
    x = U.pool_input(shape, dtype, 31)
    ho, wo = (h - 2) // stride + 1, (w - 2) // stride + 1
    dy = U.rnd((n, c, ho, wo), 32).to(dtype).float()
    ref, mag = U.pool_bwd_ref(x, dy, stride)
    got = _nchw_cpu(drn.maxpool2x2_bwd_nhwc(_nhwc_dev(x, dtype), _nhwc_dev(dy, dtype), stride))
    if stride == 2:  # routing only
        assert torch.equal(got.to(dtype), ref.to(dtype)), int((got.double() != ref).sum())
        assert (got[:, :, 2 * ho:] == 0).all() and (got[:, :, :, 2 * wo:] == 0).all()  # past the last window
    else:            # up to four dy values meet in one pixel
        bound = 3 * U.EPS32 * mag + U.e_store(dtype) * ref.abs()
        bad = (got.double() - ref).abs() > bound
        assert not bad.any(), (int(bad.sum()), float((got.double() - ref).abs().max()))
        if dtype == U.F32:
            nz = bound > 0
            _report("maxpool_bwd_s1 %s fp32" % (shape,), float(((got.double() - ref).abs()[nz] / bound[nz]).max()) if nz.any() else 0.0)


@pytest.mark.parametrize("dtype", U.DTYPES, ids=U.dname)
@pytest.mark.parametrize("n", U.ADD_SIZES)
def test_add(drn, n, dtype):
    a, b = U.rnd((n,), 41).to(dtype), U.rnd((n,), 42).to(dtype)
    got = drn.add(a.to(DEV), b.to(DEV)).cpu()
    assert torch.equal(got, a + b)


# ---- 2. Conv2d.backward_nhwc, one layer, every argument ------------------------------------------------------------------------------
def _make_conv(case, form, p):
    from drn_wsod_pytorch_amd.layers import Conv2d, FrozenBatchNorm2d

    n, h, w, cin, cout, k, stride, pad, dil = case
    norm = FrozenBatchNorm2d(cout, eps=0.0) if form == "bn" else None  # eps 0, variance 1: the folded scale IS norm.weight
    conv = Conv2d(cin, cout, kernel_size=k, stride=stride, padding=pad, dilation=dil, bias=(form == "vgg"), norm=norm)
    with torch.no_grad():
        conv.weight.copy_(p["w"])
        if form == "bn":
            conv.norm.weight.copy_(p["scale"])
            conv.norm.bias.copy_(p["bias"])
            conv.norm.running_var.fill_(1.0)
        else:
            conv.bias.copy_(p["bias"])
    return conv.to(DEV)


def _garbage_grads(conv, seed):
    conv.weight.grad = U.rnd(tuple(conv.weight.shape), seed, 100.0).to(DEV)
    if conv.bias is not None:
        conv.bias.grad = U.rnd(tuple(conv.bias.shape), seed + 1, 100.0).to(DEV)


@pytest.mark.parametrize("dtype", U.DTYPES, ids=U.dname)
@pytest.mark.parametrize("combo", U.CONV_COMBOS, ids=lambda c: "%s-relu%d-res%d-exact%d" % c)
@pytest.mark.parametrize("ci", range(len(U.CONV_CASES)))
def test_conv_backward_layer(drn, ci, combo, dtype):
    from drn_wsod_pytorch_amd import set_precision
    from drn_wsod_pytorch_amd.layers import dx_only

    case = U.CONV_CASES[ci]
    form, relu, residual, exact_g = combo
    n, h, w, cin, cout, k, stride, pad, dil = case
    tag = "case%d %s %s" % (ci, "%s-relu%d-res%d-exact%d" % combo, U.dname(dtype))
    p = U.conv_params(case, form, exact_g, 100 + ci)
    set_precision("bf16" if dtype == U.BF16 else "fp32")
    try:
        conv = _make_conv(case, form, p)
        _, scale_d, bias_d = conv.packed(dtype)
        scale = scale_d.cpu() if scale_d is not None else None
        bias = bias_d.cpu()
        if form == "bn":
            assert torch.equal(scale, p["scale"]) and torch.equal(bias, p["bias"])
        if exact_g and scale is not None:
            assert all(float(s) in (0.5, 1.0, 2.0) for s in scale)
        cp = conv.cin_pad(dtype)
        xd = _nhwc_dev(p["x"], dtype, cp)
        resd = _nhwc_dev(p["res"], dtype) if residual else None
        y = conv.run_nhwc(xd, residual=resd, relu=relu, explicit_backward=True)
        yc = _nchw_cpu(y)
        # the forward, on its own
        pre, fb = U.conv_fwd_ref(p["x"], p["w"], scale, bias, p["res"] if residual else None, stride, pad, dil, dtype)
        r_f = _report("fwd " + tag, U.worst_ratio(yc, torch.relu(pre) if relu else pre, fb))
        assert r_f <= 1.0, (tag, "forward error / bound", r_f)
        mask = None
        if relu:
            ndiff, nbad = U.mask_disagreement(pre, fb, yc)
            assert nbad == 0 and ndiff <= 1e-3 * yc.numel(), (ndiff, nbad)
            mask = yc > 0

        def check(dys_as_given, acc_tag):
            """the gradients now in .grad against the float64 sum over `dys_as_given`; the bound is the sum of the bounds"""
            refs = [U.conv_bwd_ref(p["x"], p["w"], d, mask, scale, stride, pad, dil, dtype, exact_g) for d in dys_as_given]
            dW, bW = sum(r["dW"] for r in refs), sum(r["dW_bound"] for r in refs)
            r_w = _report("dW %s %s" % (acc_tag, tag), U.worst_ratio(conv.weight.grad.cpu(), dW, bW))
            assert r_w <= 1.0, (tag, acc_tag, "dW error / bound", r_w)
            if form == "vgg":
                db, bb_ = sum(r["db"] for r in refs), sum(r["db_bound"] for r in refs)
                r_b = _report("db %s %s" % (acc_tag, tag), U.worst_ratio(conv.bias.grad.cpu(), db, bb_))
                assert r_b <= 1.0, (tag, acc_tag, "bias-gradient error / bound", r_b)
            return refs[-1]

        # (a) dy in the compute dtype, accumulate False on gradients prefilled with garbage, need_dx True at every stride
        _garbage_grads(conv, 7)
        dyA = p["dys"][0].to(dtype).float()
        dyA_d = _nhwc_dev(dyA, dtype)
        dx, d_res = conv.backward_nhwc(xd, y, dyA_d, relu, True, residual, False)
        ref = check([dyA], "first")
        assert dx.shape == xd.shape and dx.dtype == dtype
        r_x = _report("dx " + tag, U.worst_ratio(_nchw_cpu(dx, cin), ref["dx"], ref["dx_bound"]))
        assert r_x <= 1.0, (tag, "dx error / bound", r_x)
        assert (dx[..., cin:] == 0).all()
        if residual:
            assert torch.equal(_nchw_cpu(d_res).to(dtype), ref["d_res"].to(dtype))
        else:
            assert d_res is None
        # (b) a second dy, handed over as fp32 in either mode, accumulate True, need_dx False: None, and no dgrad
        dyB = p["dys"][1]
        dyB_d = _nhwc_dev(dyB, torch.float32)
        dx2, d_res2 = conv.backward_nhwc(xd, y, dyB_d, relu, False, residual, True)
        assert dx2 is None
        refB = check([dyA, dyB], "accumulated")
        if residual:
            assert torch.equal(_nchw_cpu(d_res2).to(dtype), refB["d_res"].to(dtype))
        # (c) dx_only: the same dx, bit for bit, and no gradient tensor changes
        before = [conv.weight.grad.clone()] + ([conv.bias.grad.clone()] if conv.bias is not None else [])
        with dx_only():
            dx3, _ = conv.backward_nhwc(xd, y, dyA_d, relu, True, residual, False)
        after = [conv.weight.grad] + ([conv.bias.grad] if conv.bias is not None else [])
        assert all(torch.equal(a, b) for a, b in zip(before, after))
        assert torch.equal(dx3, dx)
    finally:
        set_precision("fp32")


@pytest.mark.parametrize("kcase", U.DGRAD_KIND_CASES, ids=lambda c: "%s-%s" % (c[0], c[1]))
def test_dgrad_through_every_forward_kernel(drn, kcase):
    """Conv2d._dgrad on the smallest map that still plans to each forward kernel of the table in the module docstring"""
    from drn_wsod_pytorch_amd import set_precision
    from drn_wsod_pytorch_amd.layers import Conv2d

    kind, dt, (n, ho, wo, cin, cout, k, pad, dil) = kcase
    dtype = U.BF16 if dt == "bf16" else U.F32
    set_precision(dt)
    try:
        conv = Conv2d(cin, cout, kernel_size=k, stride=1, padding=pad, dilation=dil, bias=False)
        wt = U.rnd((cout, cin, k, k), 51, math.sqrt(2.0 / (k * k * cout)))
        with torch.no_grad():
            conv.weight.copy_(wt)
        conv = conv.to(DEV)
        g = U.rnd((n, cout, ho, wo), 52).to(dtype).float()
        gd = _nhwc_dev(g, dtype)
        cp = conv.cin_pad(dtype)
        plan = drn.conv2d_plan(gd, conv.packed_dgrad(dtype), cp, k, k, 1, dil * (k - 1) - pad, dil, None, None, dtype)
        assert U.KIND_NAMES[plan] == kind  # this map runs the kernel the case is named after
        dx = conv._dgrad(gd, (n, ho, wo, cp), dtype)  # (stride 1, "same" padding: the input map has the output's size)
        ref, bound = U.dgrad_ref(g, wt, pad, dil, dtype)
        assert dx.shape == (n, ho, wo, cp)
        r = _report("dgrad %s %s" % (kind, dt), U.worst_ratio(_nchw_cpu(dx, cin), ref, bound))
        assert r <= 1.0, (kind, dt, "dx error / bound", r)
        assert (dx[..., cin:] == 0).all()
    finally:
        set_precision("fp32")


# ---- 3. block backwards ------------------------------------------------------------------------------------------------------------------
def _check_saved_forward(blk, sv, dtype):
    """every conv of the block, forward, at its saved input: the saved output inside the forward bound of the float64 result, its
    ReLU mask the float64 mask except inside that bound"""
    kind = U.block_kind(blk)
    C = U.block_specs(blk, dtype)
    if kind == "BasicStem":
        layers = [("conv1", sv[0], sv[1], None, True), ("conv2", sv[1], sv[2], None, True), ("conv3", sv[2], sv[3], None, True)]
    elif kind == "PlainBlock":
        layers = [("conv%d" % (i + 1), sv[i], sv[i + 1], None, True) for i in range(blk.num_conv)]
    elif kind == "BasicBlock":
        x, o1, sc, out = sv
        layers = [("conv1", x, o1, None, True), ("conv2", o1, out, sc, True)]
    else:
        x, o1, o2, sc, out = sv
        layers = [("conv1", x, o1, None, True), ("conv2", o1, o2, None, True), ("conv3", o2, out, sc, True)]
    if getattr(blk, "shortcut", None) is not None:
        layers.append(("shortcut", sv[0], sv[-2], None, False))
    for name, xin, yout, res, relu in layers:
        c = C[name]
        pre, fb = U.conv_fwd_ref(xin, c["w"], c["scale"], c["bias"], res, c["stride"], c["pad"], c["dil"], dtype)
        assert U.worst_ratio(yout, torch.relu(pre) if relu else pre, fb) <= 1.0, name
        if relu:
            ndiff, nbad = U.mask_disagreement(pre, fb, yout)
            assert nbad == 0 and ndiff <= 1e-3 * yout.numel(), (name, ndiff, nbad)


@pytest.mark.parametrize("dtype", U.DTYPES, ids=U.dname)
@pytest.mark.parametrize("case", U.BLOCK_CASES, ids=lambda c: c[0])
def test_block_backward(drn, case, dtype):
    from drn_wsod_pytorch_amd import set_precision
    from drn_wsod_pytorch_amd.layers import dx_only

    bb = importlib.import_module("drn_wsod_pytorch_amd.modeling.backbone")
    name, kw, (h, w) = case
    cin = kw["cin"]
    set_precision("bf16" if dtype == U.BF16 else "fp32")
    try:
        blk = U.make_block(bb, kw, 7).to(DEV)
        params = dict(blk.named_parameters())
        for i, (pn, p_) in enumerate(sorted(params.items())):
            p_.grad = U.rnd(tuple(p_.shape), 60 + i, 100.0).to(DEV)  # garbage: accumulate=False must overwrite it
        x = U.rnd((2, cin, h, w), 8).to(dtype).float()
        xd = _nhwc_dev(x, dtype, U.cin_pad(cin, dtype))

        def read_sv():
            sv = [_nchw_cpu(t) for t in blk._sv]
            sv[0] = sv[0][:, :cin]
            return tuple(sv)

        out = blk.forward_nhwc(xd, save=True)
        sv = read_sv()
        _check_saved_forward(blk, sv, dtype)
        dy1 = U.rnd((out.shape[0], out.shape[3], out.shape[1], out.shape[2]), 9).to(dtype).float()
        dy2 = U.rnd((out.shape[0], out.shape[3], out.shape[1], out.shape[2]), 10)
        ref = [U.block_backward_chain(U.Arith("f64", dtype), blk, sv, d, True) for d in (dy1, dy2)]
        emu = [U.block_backward_chain(U.Arith("emu", dtype), blk, sv, d, True) for d in (dy1, dy2)]

        def compare(what, got, want, emulated):
            d_l2, e_l2 = U.rel_l2(got, want), U.rel_l2(emulated, want)
            d_mx, e_mx = U.rel_max(got, want), U.rel_max(emulated, want)
            msg = "BLOCK %s %s %s: rel-L2 device %.3g emulation %.3g; max/max device %.3g emulation %.3g" % (
                name, U.dname(dtype), what, d_l2, e_l2, d_mx, e_mx)
            print(msg)
            assert d_l2 <= 4 * e_l2 + 1e-6 and d_mx <= 4 * e_mx + 1e-6, msg

        # dx_only first (the CSC image-gradient passes): no gradient tensor changes and the saved activations stay
        before = {pn: p_.grad.clone() for pn, p_ in params.items()}
        with dx_only():
            dx0 = blk.backward_nhwc(_nhwc_dev(dy1, dtype), need_dx=True, accumulate=False)
        assert all(torch.equal(before[pn], p_.grad) for pn, p_ in params.items()) and blk._sv is not None
        # accumulate False, need_dx True
        dx = blk.backward_nhwc(_nhwc_dev(dy1, dtype), need_dx=True, accumulate=False)
        assert blk._sv is None and torch.equal(dx, dx0)
        assert set(params) == set(ref[0][1])
        compare("dx", _nchw_cpu(dx, cin), ref[0][0], emu[0][0])
        assert (dx[..., cin:] == 0).all()
        for pn in sorted(params):
            compare(pn, params[pn].grad.cpu(), ref[0][1][pn], emu[0][1][pn])
        # the same forward again, then an fp32 dy (the block casts it), accumulate True, need_dx False
        blk.forward_nhwc(xd, save=True)
        assert all(torch.equal(a, b) for a, b in zip(sv, read_sv()))
        none = blk.backward_nhwc(_nhwc_dev(dy2, torch.float32), need_dx=False, accumulate=True)
        assert none is None
        for pn in sorted(params):
            compare(pn + " accumulated", params[pn].grad.cpu(), ref[0][1][pn] + ref[1][1][pn],
                    emu[0][1][pn] + emu[1][1][pn])
    finally:
        set_precision("fp32")
