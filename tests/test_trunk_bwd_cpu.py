"""CPU checks of the references and bounds that test_trunk_bwd_gpu.py holds the trunk's backward kernels to (trunk_bwd_util.py):
  * the im2col_t reference equals the written-out definition; the pool inputs really hold the planted ties;
  * a plain torch emulation of the device's conv backward (fp32 arithmetic, g / d_res / dx rounded to the compute dtype) stays
    inside every bound of the single-layer tests, the bounds are not vacuous (swapped taps, one stale column, a shifted column
    scale break them), and its forward mask agrees with the float64 mask on every element;
  * the layer-by-layer float64 block chain equals float64 autograd of the whole block to 1e-12;
  * the dgrad kernel-kind table and the "smallest map" of each pinned dgrad case, re-derived with the host-only conv2d_plan.
No GPU is needed; the printed ratios (pytest -s) are the reference-side figures."""
import importlib

import pytest
import torch
import torch.nn.functional as F

import trunk_bwd_util as U
from __graft_entry__ import build


@pytest.fixture(scope="module")
def pkg():
    build()
    return importlib.import_module("drn_wsod_pytorch_amd")


@pytest.fixture(scope="module")
def bb(pkg):
    return importlib.import_module("drn_wsod_pytorch_amd.modeling.backbone")


# ---- section 1 ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", [U.IM2COL_CASES[0], U.IM2COL_CASES[1], U.IM2COL_CASES[2], U.IM2COL_CASES[5]])
def test_im2col_reference_equals_definition(case):
    n, h, w, cin, k, stride, pad, dil = case
    x = U.rnd((n, cin, h, w), 1)
    ref = U.im2col_t_ref(x, k, stride, pad, dil)
    ho, wo = U.out_hw(h, w, k, stride, pad, dil)
    assert ref.shape == (cin * k * k, n * ho * wo)
    g = torch.Generator().manual_seed(0)
    for _ in range(400):
        ci, kh, kw, b, oh, ow = [int(torch.randint(0, m, (1,), generator=g)) for m in (cin, k, k, n, ho, wo)]
        hi, wi = oh * stride + kh * dil - pad, ow * stride + kw * dil - pad
        want = float(x[b, ci, hi, wi]) if 0 <= hi < h and 0 <= wi < w else 0.0
        assert float(ref[(ci * k + kh) * k + kw, (b * ho + oh) * wo + ow]) == want


@pytest.mark.parametrize("dtype", U.DTYPES)
@pytest.mark.parametrize("shape", U.POOL_BWD_SHAPES)
def test_pool_inputs_hold_zeros_and_ties(shape, dtype):
    n, h, w, c = shape
    x = U.pool_input(shape, dtype, 11)
    assert torch.equal(x, x.to(dtype).float()) and (x >= 0).all()
    if x.numel() > 64:
        assert 0.3 < float((x == 0).float().mean()) < 0.7
    win = F.unfold(x, 2, stride=1).reshape(n, c, 4, -1)  # every stride-1 window
    mx = win.max(dim=2, keepdim=True).values
    ties = ((win == mx) & (mx > 0)).sum(dim=2) >= 2       # windows whose positive maximum is held twice
    pairs = set()
    for b, ch, p in ties.nonzero().tolist():
        pos = tuple((win[b, ch, :, p] == mx[b, ch, 0, p]).nonzero().flatten().tolist())
        pairs.add(pos[:2])
    want = 6 if (h >= 6 and w >= 10) or c >= 6 else min(c, 6)
    assert len(pairs) >= want, pairs
    if x.numel() > 64:
        assert bool(((mx == 0).sum() > 0)), "no all-zero window"
    # routing only at stride 2: the float64 gradient is one dy value or 0 - exact in the dtype
    dy = U.rnd((n, c, (h - 2) // 2 + 1, (w - 2) // 2 + 1), 12).to(dtype).float()
    dx, mag = U.pool_bwd_ref(x, dy, 2)
    assert torch.equal(dx, dx.to(dtype).double()) and torch.equal(dx.abs(), mag)
    assert (dx[:, :, 2 * ((h - 2) // 2 + 1):] == 0).all() and (dx[:, :, :, 2 * ((w - 2) // 2 + 1):] == 0).all()


# ---- section 2: the emulation stays inside the bounds, and the bounds bite ---------------------------------------------------------------
def _emulated_forward(p, case, dtype, relu, residual):
    n, h, w, cin, cout, k, stride, pad, dil = case
    y = F.conv2d(p["x"].to(dtype).float(), p["w"].to(dtype).float(), None, stride, pad, dil)
    if p["scale"] is not None:
        y = y * p["scale"].view(1, -1, 1, 1)
    y = y + p["bias"].view(1, -1, 1, 1)
    if residual:
        y = y + p["res"].to(dtype).float()
    if relu:
        y = torch.relu(y)
    return y.to(dtype).float()


@pytest.mark.parametrize("dtype", U.DTYPES)
@pytest.mark.parametrize("combo", U.CONV_COMBOS, ids=lambda c: "%s-relu%d-res%d-exact%d" % c)
@pytest.mark.parametrize("ci", range(len(U.CONV_CASES)))
def test_conv_emulation_inside_bounds(ci, combo, dtype):
    case = U.CONV_CASES[ci]
    form, relu, residual, exact_g = combo
    n, h, w, cin, cout, k, stride, pad, dil = case
    p = U.conv_params(case, form, exact_g, 100 + ci)
    y = _emulated_forward(p, case, dtype, relu, residual)
    pre, fb = U.conv_fwd_ref(p["x"], p["w"], p["scale"], p["bias"], p["res"] if residual else None, stride, pad, dil, dtype)
    if relu:
        ndiff, nbad = U.mask_disagreement(pre, fb, y)
        assert ndiff == 0 and nbad == 0, (ndiff, nbad)  # the seeds are kept so that the emulation's mask is the float64 mask
    else:
        assert U.worst_ratio(y, pre, fb) <= 1.0
    mask = (y > 0) if relu else None
    dy = p["dys"][0].to(dtype).float()
    ref = U.conv_bwd_ref(p["x"], p["w"], dy, mask, p["scale"], stride, pad, dil, dtype, exact_g)
    emu = U.emulate_conv_bwd(p["x"], p["w"], dy, mask, p["scale"], stride, pad, dil, dtype)
    rw = U.worst_ratio(emu["dW"], ref["dW"], ref["dW_bound"])
    rx = U.worst_ratio(emu["dx"], ref["dx"], ref["dx_bound"])
    rb = U.worst_ratio(emu["db"], ref["db"], ref["db_bound"])
    print("conv case %d %s %s: dW %.3f dx %.3f db %.3f of the bound" % (ci, combo, U.dname(dtype), rw, rx, rb))
    assert rw <= 1.0 and rx <= 1.0 and rb <= 1.0, (rw, rx, rb)
    assert torch.equal(emu["d_res"].double(), ref["d_res"].to(dtype).double())
    # an fp32 dy handed to a bf16 conv: the reference takes the unrounded values, g's rounding is inside e_g * mag
    if dtype == U.BF16 and not exact_g:
        dyf = p["dys"][1]
        ref = U.conv_bwd_ref(p["x"], p["w"], dyf, mask, p["scale"], stride, pad, dil, dtype, exact_g)
        emu = U.emulate_conv_bwd(p["x"], p["w"], dyf, mask, p["scale"], stride, pad, dil, dtype)
        assert U.worst_ratio(emu["dW"], ref["dW"], ref["dW_bound"]) <= 1.0
        assert U.worst_ratio(emu["dx"], ref["dx"], ref["dx_bound"]) <= 1.0
        assert torch.equal(emu["d_res"].double(), ref["d_res"].to(dtype).double())


@pytest.mark.parametrize("dtype", U.DTYPES)
@pytest.mark.parametrize("ci", [0, 1, 5])
def test_conv_bounds_bite(ci, dtype):
    """the per-element bounds are not vacuous: one swapped pair of taps in the weight gradient, one pixel column of dW's
    contraction counted twice (a stale padding column), a column scale applied to the neighbouring column each leave them"""
    case = U.CONV_CASES[ci]
    n, h, w, cin, cout, k, stride, pad, dil = case
    p = U.conv_params(case, "bn", False, 100 + ci)
    y = _emulated_forward(p, case, dtype, True, False)
    mask = y > 0
    dy = p["dys"][0].to(dtype).float()
    ref = U.conv_bwd_ref(p["x"], p["w"], dy, mask, p["scale"], stride, pad, dil, dtype, False)
    emu = U.emulate_conv_bwd(p["x"], p["w"], dy, mask, p["scale"], stride, pad, dil, dtype)
    # (a) taps kw = 0 and kw = K-1 of one kernel row swapped
    bad = emu["dW"].clone()
    bad[:, :, 0, 0], bad[:, :, 0, k - 1] = emu["dW"][:, :, 0, k - 1], emu["dW"][:, :, 0, 0]
    assert U.worst_ratio(bad, ref["dW"], ref["dW_bound"]) > 1.0
    # (b) one output pixel's contribution counted twice
    g1 = torch.zeros_like(dy)
    g1[0, :, 0, 0] = (dy * mask.float() * p["scale"].view(1, -1, 1, 1))[0, :, 0, 0]
    xr, wr = p["x"].to(dtype).float().requires_grad_(True), p["w"].to(dtype).float().requires_grad_(True)
    _, extra = torch.autograd.grad(F.conv2d(xr, wr, None, stride, pad, dil), (xr, wr), g1)
    assert U.worst_ratio(emu["dW"] + extra, ref["dW"], ref["dW_bound"]) > 1.0
    # (c) the per-column scale shifted by one column
    shifted = U.emulate_conv_bwd(p["x"], p["w"], dy, mask, p["scale"].roll(1), stride, pad, dil, dtype)
    assert U.worst_ratio(shifted["dW"], ref["dW"], ref["dW_bound"]) > 1.0
    assert U.worst_ratio(shifted["dx"], ref["dx"], ref["dx_bound"]) > 1.0
    # (for comparison, the same two errors in the whole-tensor max-norm measure of test_conv_backward)
    relmax = lambda a, b: float((a.double() - b).abs().max() / b.abs().max())
    print("swapped taps: max-norm error %.3g, doubled pixel: %.3g" % (relmax(bad, ref["dW"]), relmax(emu["dW"] + extra, ref["dW"])))


# ---- section 3: the layer-by-layer chain is the gradient of the block --------------------------------------------------------------------
@pytest.mark.parametrize("need_dx", [True, False])
@pytest.mark.parametrize("case", U.BLOCK_CASES, ids=lambda c: c[0])
def test_block_chain_equals_whole_block_autograd(bb, case, need_dx):
    name, kw, (h, w) = case
    blk = U.make_block(bb, kw, 7)
    x = U.rnd((2, kw["cin"], h, w), 8).double().requires_grad_(True)
    # whole-block autograd: the same forward with the parameters as float64 leaves
    convs = U.block_convs(blk)
    specs = U.block_specs(blk, U.F32)
    leaves = {}
    for n_ in convs:
        c = specs[n_]
        c["w"] = c["w"].double().requires_grad_(True)
        if c["has_bias_grad"]:
            c["bias"] = c["bias"].double().requires_grad_(True)
        leaves[n_] = (c["w"], c["bias"] if c["has_bias_grad"] else None)
    sv, out = U.block_forward64(blk, x, specs=specs)
    dy = U.rnd(tuple(out.shape), 9).double()
    wanted = [x] + [leaves[n_][0] for n_ in convs] + [leaves[n_][1] for n_ in convs if leaves[n_][1] is not None]
    got = torch.autograd.grad(out, wanted, dy)
    want = {"x": got[0]}
    for i, n_ in enumerate(convs):
        want[n_ + ".weight"] = got[1 + i]
    for j, n_ in enumerate([n_ for n_ in convs if leaves[n_][1] is not None]):
        want[n_ + ".bias"] = got[1 + len(convs) + j]
    # the chain at the same (CPU-computed, float64) activations
    A = U.Arith("f64", U.F32)
    dx, grads = U.block_backward_chain(A, blk, tuple(t.detach() for t in sv), dy, need_dx)
    assert set(grads) == set(want) - {"x"}
    for n_, g in grads.items():
        assert U.rel_max(g, want[n_]) <= 1e-12, (n_, U.rel_max(g, want[n_]))
    if need_dx:
        assert U.rel_max(dx, want["x"]) <= 1e-12
    else:
        assert dx is None


@pytest.mark.parametrize("dtype", U.DTYPES)
@pytest.mark.parametrize("case", U.BLOCK_CASES, ids=lambda c: c[0])
def test_block_storage_emulation_error(bb, case, dtype):
    """the emulation's own error against the float64 chain (what sizes the GPU tolerance): printed per tensor; it must be small
    but, in bf16, not zero - a tolerance of 4 x 0 would be no tolerance"""
    name, kw, (h, w) = case
    blk = U.make_block(bb, kw, 7)
    x = U.rnd((2, kw["cin"], h, w), 8).to(dtype).double()
    sv, out = U.block_forward64(blk, x, dtype)
    sv = tuple(t.to(dtype).float() for t in sv)  # as the device saves them
    dy = U.rnd(tuple(out.shape), 9).to(dtype).float()
    dx64, g64 = U.block_backward_chain(U.Arith("f64", dtype), blk, sv, dy, True)
    dxe, ge = U.block_backward_chain(U.Arith("emu", dtype), blk, sv, dy, True)
    ge["dx"], g64["dx"] = dxe, dx64
    for n_ in sorted(g64):
        l2, mx = U.rel_l2(ge[n_], g64[n_]), U.rel_max(ge[n_], g64[n_])
        print("%s %s %s: emulation rel-L2 %.3g max/max %.3g" % (name, U.dname(dtype), n_, l2, mx))
        assert l2 <= (2e-2 if dtype == U.BF16 else 1e-5) and mx <= (2e-2 if dtype == U.BF16 else 1e-5)
    if dtype == U.BF16:
        assert U.rel_l2(dxe, dx64) > 1e-4


# ---- section 2b: the dgrad kernel-kind table ---------------------------------------------------------------------------------------------
def test_dgrad_kind_table(pkg):
    ops = importlib.import_module("drn_wsod_pytorch_amd.ops")
    assert U.trunk_dgrad_kinds(ops, cus=256) == U.DGRAD_KINDS
    reached = {(k, dt) for (trunk, dt), kinds in U.DGRAD_KINDS.items() for k in kinds}
    assert {(k, dt) for k, dt, _ in U.DGRAD_KIND_CASES} == reached  # one pinned case per kind and dtype of the table
    table_geos = {(dt, g[3:]) for trunk in ("r50c4", "r18dc5", "vgg16") for dt in ("bf16", "fp32")
                  for _, _, g in U.trunk_dgrad_convs(trunk)}
    for kind, dt, (n, ho, wo, cin, cout, k, pad, dil) in U.DGRAD_KIND_CASES:
        dtype = U.BF16 if dt == "bf16" else U.F32
        assert (dt, (cin, cout, k, pad, dil)) in table_geos  # a layer of the trunks, not an invented one
        assert U.KIND_NAMES[U.dgrad_plan_kind(ops, n, ho, wo, cin, cout, k, pad, dil, dtype, 256)] == kind
        if kind in U.DGRAD_KIND_THRESHOLDED:  # ... and one step smaller it is another kernel's
            assert U.KIND_NAMES[U.dgrad_plan_kind(ops, n, ho - 1, wo - 1, cin, cout, k, pad, dil, dtype, 256)] != kind
