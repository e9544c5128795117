"""Plain float64 references, error bounds and case tables for the trunk's explicit backward
(Conv2d.backward_nhwc / _dgrad, the block backwards of modeling/backbone.py, and im2col_t / maxpool2x2_bwd / add of pool.hip).

Everything here runs on the CPU with torch only.  Operands are first rounded to the compute dtype (`q`), then all reference
arithmetic is float64.  ReLU masks and pool routing are taken from SAVED forward tensors handed in by the caller (the device's
own `y` / `blk._sv` in the GPU tests), so the reference is the exact gradient linearised at the activations that were really
saved and a pre-activation within rounding of zero cannot decide a test.

Bounds (eps32 = 2^-24; h16 = 2^-8, half a bf16 ulp relative to the value):
  * accumulation of a contraction of length L with magnitude mag = sum|a||b|:  4 eps32 sqrt(L) mag + 1e-6  (the GEMM bound of
    test_gemm_nt / test_gemm_full_size_sampled); mag comes from the same float64 call on |x|, |w|, |g|;
  * a result stored in bf16 adds h16 |ref|;
  * g = dy * scale * mask is stored in the compute dtype in front of both GEMMs: with scales from {0.5, 1, 2} and a dy
    representable in the dtype ("exact g") that store does not round; with general scales it adds e_g mag, e_g = eps32 (fp32) or
    h16 (bf16), to the dW and dx bounds.
"""
import math

import torch
import torch.nn.functional as F

EPS32 = 2.0 ** -24
H16 = 2.0 ** -8
F32, BF16 = torch.float32, torch.bfloat16
DTYPES = [F32, BF16]


def dname(dtype):
    return "bf16" if dtype == BF16 else "fp32"


def q(x, dtype):
    """the value an operand has once stored in the compute dtype, as float64"""
    return x.to(dtype).double()


def rnd(shape, seed, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(shape, generator=g, dtype=torch.float32) * scale


def e_store(dtype):
    return H16 if dtype == BF16 else 0.0


def e_g(dtype, exact_g):
    return 0.0 if exact_g else (H16 if dtype == BF16 else EPS32)


def acc_bound(L, mag):
    return 4 * EPS32 * math.sqrt(L) * mag + 1e-6


def worst_ratio(got, ref, bound):
    """max |got - ref| / bound, as a float (<= 1 passes)"""
    return float(((got.double() - ref.double()).abs() / bound).max())


# ---- case tables -----------------------------------------------------------------------------------------------------------------
# (N, H, W, Cin, k, stride, pad, dil); x is stored with cin_pad(dtype) channels
IM2COL_CASES = [
    (2, 9, 11, 16, 3, 1, 1, 1),    # P = 198: ragged last 64-pixel tile, an image boundary inside a tile
    (1, 8, 8, 72, 3, 1, 2, 2),     # P = 64: exactly one tile; second channel tile holds 8 of 64; dilation 2
    (1, 21, 19, 3, 3, 2, 1, 1),    # ldc 4 / 8 > Cin, stride 2 on odd sizes, P = 110
    (1, 20, 22, 3, 3, 2, 1, 1),    # the same on even sizes
    (3, 7, 9, 136, 1, 1, 0, 1),    # 1x1, three channel tiles, P = 189
    (1, 5, 5, 8, 3, 1, 0, 1),      # pad 0, P = 9 < 64
]

# (N, H, W, C)
POOL_BWD_SHAPES = [(2, 11, 14, 24), (1, 12, 13, 3), (1, 2, 2, 8), (1, 3, 2, 136),
                   (2, 64, 65, 64)]  # 532480 elements > the 2048 x 256 span of the grid: the grid-stride loop runs twice

ADD_SIZES = [1, 255, 256, 259, 524288 + 259]

# (N, H, W, Cin, Cout, k, stride, pad, dil)
CONV_CASES = [
    (2, 9, 11, 16, 24, 3, 1, 1, 1),      # P = 198
    (2, 13, 17, 72, 40, 3, 1, 2, 2),     # dilation, ragged Cout and Cin * 9 = 648
    (1, 21, 19, 3, 8, 3, 2, 1, 1),       # the stem conv, odd sizes, padded input channels
    (1, 20, 22, 3, 8, 3, 2, 1, 1),       # the same on even sizes
    (3, 7, 9, 136, 64, 1, 1, 0, 1),      # 1x1
    (1, 33, 31, 64, 136, 3, 1, 1, 1),    # P = 1023, Cout = 2 * 64 + 8
]
# the argument combinations every conv case runs: (form, relu, residual, exact_g)
#   form "bn": FrozenBatchNorm2d scale, no conv bias; form "vgg": bias=True and no norm (no scale: "general" only means that dy is
#   not on the coarse grid, so the bias-gradient sums round, and that an fp32 dy is rounded when g is stored)
CONV_COMBOS = [("bn", True, False, True), ("bn", True, False, False), ("bn", False, False, False), ("bn", True, True, False),
               ("bn", False, True, True), ("vgg", True, False, True), ("vgg", True, False, False)]


def cin_pad(cin, dtype):
    qn = 8 if dtype == BF16 else 4
    return (cin + qn - 1) // qn * qn


def out_hw(h, w, k, stride, pad, dil):
    return (h + 2 * pad - dil * (k - 1) - 1) // stride + 1, (w + 2 * pad - dil * (k - 1) - 1) // stride + 1


# ---- section 1: references of the pool.hip kernels --------------------------------------------------------------------------------
def im2col_t_ref(x_nchw, k, stride, pad, dil):
    """x [N, C, H, W] (already in the dtype) -> [C*k*k, N*Ho*Wo]: row (ci*k + kh)*k + kw, column (n*Ho + ho)*Wo + wo.
    F.unfold is pure data movement: exact in any dtype (done in float32, which holds every bf16 value)."""
    n = x_nchw.shape[0]
    u = F.unfold(x_nchw.float(), k, dilation=dil, padding=pad, stride=stride)  # [N, C*k*k, Ho*Wo]
    return u.permute(1, 0, 2).reshape(u.shape[1], n * u.shape[2]).to(x_nchw.dtype)


def pool_input(shape, dtype, seed):
    """what the trunk feeds the pool backward: relu(randn) rounded to the dtype (about half exact zeros: all-zero windows and
    zero / positive ties), with equal positive maxima planted at each of the 6 position pairs of a window where the map has room"""
    n, h, w, c = shape
    x = torch.relu(rnd((n, c, h, w), seed)).to(dtype).float()
    pairs = [(a, b) for a in range(4) for b in range(a + 1, 4)]
    roomy = h >= 6 and w >= 10  # six windows 4 apart: they share no pixel even at stride 1
    for i, (a, b) in enumerate(pairs):
        if roomy:
            h0, w0, ch = 4 * (i // 3), 4 * (i % 3), slice(None)
        elif i < c:
            h0, w0, ch = 0, 0, slice(i, i + 1)  # small maps: one channel per pair, all in the first window
        else:
            continue
        x[0, ch, h0:h0 + 2, w0:w0 + 2] = 0.25
        x[0, ch, h0 + a // 2, w0 + a % 2] = 3.0
        x[0, ch, h0 + b // 2, w0 + b % 2] = 3.0
    return x


def pool_bwd_ref(x, dy, stride):
    """float64 autograd of F.max_pool2d(x, 2, stride) -> (dx, sum of |dy| routed to each pixel)"""
    xr = x.double().requires_grad_(True)
    y = F.max_pool2d(xr, 2, stride)
    dx, = torch.autograd.grad(y, xr, dy.double(), retain_graph=True)
    mag, = torch.autograd.grad(y, xr, dy.double().abs())
    return dx, mag


# ---- section 2: one conv layer -----------------------------------------------------------------------------------------------------
def conv_fwd_ref(x, w, scale, bias, res, stride, pad, dil, dtype):
    """float64 pre-activation conv(x, w) * scale + bias (+ res) of dtype-rounded operands, and the forward bound
    4 eps32 sqrt(Cin k k) mag |scale| + 1e-6 (+ h16 |ref| in bf16) used for the mask check"""
    xq, wq = q(x, dtype), q(w, dtype)
    pre = F.conv2d(xq, wq, None, stride, pad, dil)
    mag = F.conv2d(xq.abs(), wq.abs(), None, stride, pad, dil)
    sc = scale.double().view(1, -1, 1, 1) if scale is not None else torch.ones(1, dtype=torch.float64).view(1, 1, 1, 1)
    pre = pre * sc
    if bias is not None:
        pre = pre + bias.double().view(1, -1, 1, 1)
    if res is not None:
        pre = pre + q(res, dtype)
    L = w.shape[1] * w.shape[2] * w.shape[3]
    bound = acc_bound(L, mag * sc.abs()) + e_store(dtype) * pre.abs()
    return pre, bound


def mask_disagreement(pre, bound, y_saved):
    """(number of outputs whose saved mask y > 0 differs from the float64 mask, number of those that the forward bound does NOT
    explain).  The second must be 0; the first at most 0.1 % of the outputs."""
    diff = (y_saved > 0) != (pre > 0)
    return int(diff.sum()), int((diff & (pre.abs() > bound)).sum())


def conv_bwd_ref(x, w, dy, mask, scale, stride, pad, dil, dtype, exact_g):
    """The exact gradient of conv(x, w) * scale (+ bias) (+ res) -> relu, linearised at the saved mask.
    x [N,Cin,H,W], w [Cout,Cin,k,k] (rounded here to the dtype), dy [N,Cout,Ho,Wo] with the values the device is handed (the
    caller rounds it when it hands the device a dy in the compute dtype), mask bool like dy or None (no ReLU), scale [Cout] or None.  Returns a dict of float64 tensors: dW, dW_bound, dx, dx_bound, db, db_bound, d_res.
    d_res = dy * mask is what the residual input gets (no scale), compared bit-exactly after rounding to the dtype."""
    xq, wq, dyq = q(x, dtype), q(w, dtype), dy.double()
    m = mask.double() if mask is not None else torch.ones_like(dyq)
    d_res = dyq * m
    sc = scale.double().view(1, -1, 1, 1) if scale is not None else torch.ones(1, dtype=torch.float64).view(1, 1, 1, 1)
    g = d_res * sc
    n, cout, ho, wo = g.shape
    P = n * ho * wo
    k = w.shape[2]

    def grads(xx, ww, gg):
        xx, ww = xx.clone().requires_grad_(True), ww.clone().requires_grad_(True)
        return torch.autograd.grad(F.conv2d(xx, ww, None, stride, pad, dil), (xx, ww), gg)

    dx, dW = grads(xq, wq, g)
    mx, mW = grads(xq.abs(), wq.abs(), g.abs())
    eg = e_g(dtype, exact_g)
    out = dict(dW=dW, dx=dx, d_res=d_res, g=g)
    out["dW_bound"] = acc_bound(P, mW) + eg * mW
    out["dx_bound"] = acc_bound(k * k * cout, mx) + eg * mx + e_store(dtype) * dx.abs()
    out["db"] = d_res.sum(dim=(0, 2, 3))          # bias gradient of the VGG form (no scale)
    out["db_bound"] = acc_bound(P, d_res.abs().sum(dim=(0, 2, 3)))
    return out


def emulate_conv_bwd(x, w, dy, mask, scale, stride, pad, dil, dtype):
    """the device's chain in plain torch: float32 arithmetic, g and dx rounded to the compute dtype where the device stores them"""
    xf, wf = x.to(dtype).float(), w.to(dtype).float()
    g = dy.float()
    if mask is not None:
        g = g * mask.float()
    d_res = g.to(dtype).float()
    if scale is not None:
        g = g * scale.float().view(1, -1, 1, 1)
    g = g.to(dtype).float()
    xr, wr = xf.clone().requires_grad_(True), wf.clone().requires_grad_(True)
    dx, dW = torch.autograd.grad(F.conv2d(xr, wr, None, stride, pad, dil), (xr, wr), g)
    return dict(dW=dW, dx=dx.to(dtype).float(), d_res=d_res, db=d_res.sum(dim=(0, 2, 3)))


def conv_params(case, form, exact_g, seed):
    """weights / scale / bias / input / two output gradients of one conv case, float32 on the CPU.
    exact g: scales from {0.5, 1, 2} and dy on a coarse binary grid (multiples of 1/8 up to +-4: exact in bf16, and so is every
    product with the scale); general: scale = 0.5 + rand."""
    n, h, w_, cin, cout, k, stride, pad, dil = case
    g = torch.Generator().manual_seed(seed)
    wt = torch.randn((cout, cin, k, k), generator=g) * math.sqrt(2.0 / (cin * k * k))
    x = torch.randn((n, cin, h, w_), generator=g)
    ho, wo = out_hw(h, w_, k, stride, pad, dil)
    if form == "vgg":
        scale, bias = None, torch.randn((cout,), generator=g) * 0.1
    else:
        scale = (torch.tensor([0.5, 1.0, 2.0])[torch.randint(0, 3, (cout,), generator=g)] if exact_g
                 else 0.5 + torch.rand((cout,), generator=g))
        bias = torch.randn((cout,), generator=g) * 0.1
    res = torch.randn((n, cout, ho, wo), generator=g)
    dys = []
    for _ in range(2):
        d = torch.randn((n, cout, ho, wo), generator=g)
        dys.append((d * 8).round().clamp(-32, 32) / 8 if exact_g else d)
    return dict(w=wt, x=x, scale=scale, bias=bias, res=res, dys=dys, ho=ho, wo=wo)


# ---- section 2b: the forward kernels the dgrad convs of the trainable trunks reach ---------------------------------------------------
KIND_NAMES = {1: "PATCH_C64", 2: "PP256", 3: "PP8", 4: "PP8_WIDE", 5: "RING_64", 6: "RING_128", 7: "K2", 8: "KS", 9: "TILED_64",
              10: "TILED_128X64", 11: "TILED_128"}


def dgrad_plan_kind(ops, n, ho, wo, cin, cout, k, pad, dil, dtype, cus=0):
    """the CONV_KIND_* that serves the dgrad conv of a stride-1 Conv2d(cin, cout, k, padding=pad, dilation=dil) whose output is
    [n, ho, wo, cout]: conv2d_nhwc(g, packed_dgrad, cin_pad, k, k, 1, dil*(k-1) - pad, dil) - host-only"""
    cp = cin_pad(cin, dtype)
    g = torch.empty((n, ho, wo, cout), dtype=dtype)
    wd = torch.empty((cp, ops.kpad(k * k * cout, dtype)), dtype=dtype)
    return ops.conv2d_plan(g, wd, cp, k, k, 1, dil * (k - 1) - pad, dil, None, None, dtype, cus=cus)


def trunk_dgrad_convs(trunk, hw=(224, 224)):
    """[(unit, conv name, (n, ho, wo, cin, cout, k, pad, dil))] of every dgrad conv the training backward of `trunk` launches at
    the bench image size (N = 1): r50c4 (FREEZE_AT 2), r18dc5 (FREEZE_AT 1), vgg16 (FREEZE_AT 0, dilated conv5).  The first
    trainable unit gives no gradient to its input (need_dx False): its input-facing convs run no dgrad.  A strided conv would
    spread g first; none of the trainable units here has one."""
    H, W = hw
    half = lambda v: (v + 2 - 2 - 1) // 2 + 1
    pool = lambda v, s: (v - 2) // s + 1
    out = []
    if trunk == "vgg16":
        h, w, cin = H, W, 3
        for i, (cout, nconv) in enumerate(((64, 2), (128, 2), (256, 3), (512, 3), (512, 3))):
            dil = 2 if i == 4 else 1
            for j in range(nconv):
                if not (i == 0 and j == 0):
                    out.append(("plain%d" % (i + 1), "conv%d" % (j + 1), (1, h, w, cin, cout, 3, dil, dil)))
                cin = cout
            if i < 3:
                h, w = pool(h, 2), pool(w, 2)
            elif i == 3:
                h, w = pool(h, 1), pool(w, 1)
        return out
    depth, dc5, first_stage = (50, False, 3) if trunk == "r50c4" else (18, True, 2)
    h, w = pool(half(H), 2), pool(half(W), 2)
    cin, cout, bc = 64, 64 if depth == 18 else 256, 64
    nblocks = {18: [2, 2, 2, 2], 50: [3, 4, 6, 3]}[depth]
    for si, stage in enumerate((2, 3, 4, 5) if dc5 else (2, 3, 4)):
        dil = 2 if dc5 and stage >= 4 else 1
        for b in range(nblocks[si]):
            ci = cin if b == 0 else cout
            first_unit = stage == first_stage and b == 0
            name = "res%d.%d" % (stage, b)
            if stage >= first_stage:
                if depth == 18:
                    convs = [("conv1", ci, cout, 3, dil, not first_unit), ("conv2", cout, cout, 3, dil, True)]
                else:
                    convs = [("conv1", ci, bc, 1, 1, not first_unit), ("conv2", bc, bc, 3, dil, True), ("conv3", bc, cout, 1, 1, True)]
                if ci != cout:
                    convs.append(("shortcut", ci, cout, 1, 1, not first_unit))
                for cname, a, o, k, d, has_dx in convs:
                    if has_dx:
                        out.append((name, cname, (1, h, w, a, o, k, d * (k // 2), d)))
        if stage == 2:
            h, w = pool(h, 2), pool(w, 2)
        elif stage == 3:
            h, w = (pool(h, 1), pool(w, 1)) if dc5 else (pool(h, 2), pool(w, 2))
        cin, cout, bc = cout, cout * 2, bc * 2
    return out


def trunk_dgrad_kinds(ops, cus=256):
    """{(trunk, dtype name): sorted list of kind names}"""
    table = {}
    for trunk in ("r50c4", "r18dc5", "vgg16"):
        for dtype in (BF16, F32):
            kinds = {dgrad_plan_kind(ops, n, ho, wo, cin, cout, k, pad, dil, dtype, cus)
                     for _, _, (n, ho, wo, cin, cout, k, pad, dil) in trunk_dgrad_convs(trunk)}
            table[(trunk, dname(dtype))] = sorted(KIND_NAMES[kd] for kd in kinds)
    return table


# ---- section 3: block backwards, layer by layer ----------------------------------------------------------------------------------------
# The chain below is written from the reference's forward (resnet_ws.py BasicStem / BasicBlock / BottleneckBlock, vgg.py PlainBlock),
# not from backbone.py: every layer is a local autograd call of F.conv2d / F.max_pool2d at the SAVED activations, and the wiring -
# pool backward in front of the last conv, the ReLU mask of `out` feeding both the residual conv and the shortcut, the sum of the
# two input gradients - is stated here.  Two arithmetics run the same chain:
#   "f64": float64 throughout, nothing rounded - the reference;
#   "emu": float32 arithmetic with every tensor the device stores (g, d_res, each dx, the pool dx, the add) rounded to the compute
#          dtype - the storage emulation whose own error against "f64" sizes the tolerance.
class Arith:
    def __init__(self, mode, dtype):
        assert mode in ("f64", "emu")
        self.mode, self.dtype = mode, dtype
        self.ft = torch.float64 if mode == "f64" else torch.float32

    def val(self, t):
        return t.to(self.ft)

    def store(self, t):
        return t if self.mode == "f64" else t.to(self.dtype).to(self.ft)


def conv_spec(m, dtype):
    """what a Conv2d module computes, as plain CPU tensors: weight rounded to the dtype, folded FrozenBN scale / bias or the conv bias"""
    w = m.weight.detach().cpu().to(dtype).float()
    if m.norm is not None:
        scale, bias = [t.detach().cpu().float() for t in m.norm.folded()]
    else:
        scale, bias = None, (m.bias.detach().cpu().float() if m.bias is not None else None)
    return dict(w=w, scale=scale, bias=bias, stride=m.stride[0], pad=m.padding[0], dil=m.dilation[0],
                has_bias_grad=m.norm is None and m.bias is not None)


def layer_conv_bwd(A, c, x, y_saved, d, relu, need_dx, residual):
    """one conv layer at its saved input x and saved output y_saved (mask y > 0): -> (dx or None, dW, db or None, d_res or None)"""
    d = A.val(d)
    if relu:
        d = d * A.val(y_saved > 0)
    d_res = A.store(d) if residual else None
    db = d.sum(dim=(0, 2, 3)) if c["has_bias_grad"] else None
    g = A.store(d * A.val(c["scale"]).view(1, -1, 1, 1) if c["scale"] is not None else d)
    xr, wr = A.val(x).clone().requires_grad_(True), A.val(c["w"]).clone().requires_grad_(True)
    dx, dW = torch.autograd.grad(F.conv2d(xr, wr, None, c["stride"], c["pad"], c["dil"]), (xr, wr), g)
    return (A.store(dx) if need_dx else None), dW, db, d_res


def layer_pool_bwd(A, x_saved, d, stride):
    xr = A.val(x_saved).clone().requires_grad_(True)
    dx, = torch.autograd.grad(F.max_pool2d(xr, 2, stride), xr, A.val(d))
    return A.store(dx)


def block_kind(blk):
    return type(blk).__name__


def block_convs(blk):
    names = [n for n in ("conv1", "conv2", "conv3", "conv4", "shortcut") if getattr(blk, n, None) is not None]
    return names


def block_specs(blk, dtype):
    return {n: conv_spec(getattr(blk, n), dtype) for n in block_convs(blk)}


def block_backward_chain(A, blk, sv, dy, need_dx, specs=None):
    """-> (dx or None, {"conv1.weight": dW, "conv1.bias": db, ...}).  `sv`: the block's saved activations as NCHW CPU tensors in
    the order the forward produced them (stem: x, o1, o2, o3; basic: x, o1, sc, out; bottleneck: x, o1, o2, sc, out; plain: x, a1 ..)
    `dy` enters in the compute dtype (the blocks cast an fp32 gradient first)."""
    kind = block_kind(blk)
    dtype = A.dtype
    C = specs or block_specs(blk, dtype)
    grads = {}

    def conv(name, x, y, d, relu, ndx, residual=False):
        dx, dW, db, d_res = layer_conv_bwd(A, C[name], x, y, d, relu, ndx, residual)
        grads[name + ".weight"] = dW
        if db is not None:
            grads[name + ".bias"] = db
        return dx, d_res

    d = A.store(A.val(dy.to(dtype)))
    if kind == "BasicStem":
        x, o1, o2, o3 = sv
        d = layer_pool_bwd(A, o3, d, 2)
        d, _ = conv("conv3", o2, o3, d, True, True)
        d, _ = conv("conv2", o1, o2, d, True, True)
        d, _ = conv("conv1", x, o1, d, True, need_dx)
        return d, grads
    if kind == "PlainBlock":
        if blk.has_pool:
            d = layer_pool_bwd(A, sv[-1], d, blk.pool_stride)
        for i in range(blk.num_conv - 1, -1, -1):
            d, _ = conv("conv%d" % (i + 1), sv[i], sv[i + 1], d, True, need_dx or i > 0)
        return d, grads
    if kind == "BasicBlock":
        x, o1, sc, out = sv
        main = [("conv2", o1, out), ("conv1", x, o1)]
    else:
        assert kind == "BottleneckBlock"
        x, o1, o2, sc, out = sv
        main = [("conv3", o2, out), ("conv2", o1, o2), ("conv1", x, o1)]
    if blk.has_pool:
        d = layer_pool_bwd(A, out, d, blk.pool_stride)
    d_sc = None
    for j, (name, xin, yout) in enumerate(main):
        last = j == len(main) - 1
        d, dr = conv(name, xin, yout, d, True, need_dx or not last, residual=(j == 0))
        if j == 0:
            d_sc = dr  # relu(conv + shortcut): the shortcut branch gets dy * mask(out), without the conv's scale
    if blk.shortcut is not None:
        dxs, _ = conv("shortcut", x, sc, d_sc, False, need_dx)
    else:
        dxs = d_sc
    return (A.store(d + dxs) if need_dx else None), grads


def block_forward64(blk, x, dtype=F32, specs=None):
    """float64 forward of the block on the CPU, written from the reference: -> (saved activations in _sv order, output).  With
    `dtype` bf16 the weights are the bf16-rounded ones; activations stay float64 (the CPU test's whole-block autograd)."""
    kind = block_kind(blk)
    C = specs or block_specs(blk, dtype)

    def conv(name, t, res=None, relu=True):
        c = C[name]
        y = F.conv2d(t, c["w"].double(), None, c["stride"], c["pad"], c["dil"])
        if c["scale"] is not None:
            y = y * c["scale"].double().view(1, -1, 1, 1)
        if c["bias"] is not None:
            y = y + c["bias"].double().view(1, -1, 1, 1)
        if res is not None:
            y = y + res
        return torch.relu(y) if relu else y

    if kind == "BasicStem":
        o1 = conv("conv1", x); o2 = conv("conv2", o1); o3 = conv("conv3", o2)
        return (x, o1, o2, o3), F.max_pool2d(o3, 2, 2)
    if kind == "PlainBlock":
        acts = [x]
        for i in range(blk.num_conv):
            acts.append(conv("conv%d" % (i + 1), acts[-1]))
        return tuple(acts), (F.max_pool2d(acts[-1], 2, blk.pool_stride) if blk.has_pool else acts[-1])
    sc = conv("shortcut", x, relu=False) if blk.shortcut is not None else x
    if kind == "BasicBlock":
        o1 = conv("conv1", x)
        out = conv("conv2", o1, res=sc)
        sv = (x, o1, sc, out)
    else:
        o1 = conv("conv1", x); o2 = conv("conv2", o1)
        out = conv("conv3", o2, res=sc)
        sv = (x, o1, o2, sc, out)
    return sv, (F.max_pool2d(out, 2, blk.pool_stride) if blk.has_pool else out)


def rel_l2(a, ref):
    a, ref = a.double(), ref.double()
    return float((a - ref).norm() / max(float(ref.norm()), 1e-30))


def rel_max(a, ref):
    a, ref = a.double(), ref.double()
    return float((a - ref).abs().max() / max(float(ref.abs().max()), 1e-30))


# block cases: (name, constructor kwargs, (H, W)); N = 2, FrozenBN with random statistics, channels 8 .. 72
BLOCK_CASES = [
    ("stem_odd", dict(cls="BasicStem", cin=3, cout=16), (21, 19)),
    ("stem_even", dict(cls="BasicStem", cin=3, cout=16), (20, 22)),
    ("basic_proj_pool2", dict(cls="BasicBlock", cin=16, cout=24, stride=2, dilation=1, has_pool=True), (13, 17)),
    ("basic_id_nopool_dil2", dict(cls="BasicBlock", cin=24, cout=24, stride=1, dilation=2, has_pool=False), (11, 14)),
    ("basic_id_pool1_dil2", dict(cls="BasicBlock", cin=16, cout=16, stride=1, dilation=2, has_pool=True), (12, 9)),
    ("bottle_proj_pool1_dil2", dict(cls="BottleneckBlock", cin=24, cout=72, mid=8, stride=1, dilation=2, has_pool=True), (14, 11)),
    ("bottle_id_pool2", dict(cls="BottleneckBlock", cin=40, cout=40, mid=16, stride=2, dilation=1, has_pool=True), (17, 24)),
    ("bottle_proj_nopool", dict(cls="BottleneckBlock", cin=16, cout=64, mid=16, stride=1, dilation=1, has_pool=False), (9, 10)),
    ("plain2_pool2", dict(cls="PlainBlock", cin=3, cout=16, num_conv=2, stride=2, dilation=1, has_pool=True), (15, 18)),
    ("plain3_dil2", dict(cls="PlainBlock", cin=16, cout=24, num_conv=3, stride=1, dilation=2, has_pool=False), (12, 13)),
]


def make_block(backbone_mod, kw, seed):
    """build a block of modeling/backbone.py (as a parameter container; on the CPU) with seeded weights and FrozenBN statistics"""
    kw = dict(kw)
    cls = kw.pop("cls")
    if cls == "BasicStem":
        blk = backbone_mod.BasicStem(kw["cin"], kw["cout"], norm="FrozenBN")
    elif cls == "BasicBlock":
        blk = backbone_mod.BasicBlock(kw["cin"], kw["cout"], stride=kw["stride"], norm="FrozenBN", dilation=kw["dilation"],
                                      has_pool=kw["has_pool"])
    elif cls == "BottleneckBlock":
        blk = backbone_mod.BottleneckBlock(kw["cin"], kw["cout"], bottleneck_channels=kw["mid"], stride=kw["stride"], norm="FrozenBN",
                                           dilation=kw["dilation"], has_pool=kw["has_pool"])
    else:
        blk = backbone_mod.PlainBlock(kw["cin"], kw["cout"], num_conv=kw["num_conv"], dilation=kw["dilation"], stride=kw["stride"],
                                      has_pool=kw["has_pool"])
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for name in block_convs(blk):
            m = getattr(blk, name)
            fan = m.weight.shape[1] * m.weight.shape[2] * m.weight.shape[3]
            m.weight.copy_(torch.randn(m.weight.shape, generator=g) * math.sqrt(2.0 / fan))
            if m.bias is not None:
                m.bias.copy_(torch.randn(m.bias.shape, generator=g) * 0.1)
            if m.norm is not None:
                m.norm.weight.copy_(0.5 + torch.rand(m.norm.weight.shape, generator=g))
                m.norm.bias.copy_(torch.randn(m.norm.bias.shape, generator=g) * 0.1)
                m.norm.running_mean.copy_(torch.randn(m.norm.bias.shape, generator=g) * 0.1)
                m.norm.running_var.copy_(0.5 + torch.rand(m.norm.bias.shape, generator=g))
    return blk


# ---- the dgrad kernel-kind table (recorded with conv2d_plan on a 256-CU device, default knobs; test_trunk_bwd_cpu re-derives it) ----
DGRAD_KINDS = {
    ("r50c4", "bf16"): ["KS", "TILED_64"],
    ("r50c4", "fp32"): ["KS", "TILED_64"],
    ("r18dc5", "bf16"): ["K2", "KS", "TILED_64"],
    ("r18dc5", "fp32"): ["K2", "KS", "TILED_64"],
    ("vgg16", "bf16"): ["K2", "KS", "PATCH_C64", "RING_64"],
    ("vgg16", "fp32"): ["K2", "KS", "TILED_128X64", "TILED_64"],
}
# one dgrad case per (kind, dtype) of the table: a layer geometry of the table that reaches the kind, on the smallest map (h x h+1,
# N = 1) that still plans to it.  KS and TILED_64 have no lower threshold (they still serve a 1 x 2 map): they run on 5 x 7, the
# smallest map with interior, edge and corner pixels for a 3x3 tap set.  (kind, dtype name, (n, ho, wo, cin, cout, k, pad, dil))
DGRAD_KIND_CASES = [
    ("KS", "bf16", (1, 5, 7, 128, 128, 3, 1, 1)),
    ("KS", "fp32", (1, 5, 7, 128, 128, 3, 1, 1)),
    ("TILED_64", "bf16", (1, 5, 7, 64, 128, 1, 0, 1)),
    ("TILED_64", "fp32", (1, 5, 7, 64, 128, 1, 0, 1)),
    ("K2", "bf16", (1, 23, 24, 512, 512, 3, 2, 2)),
    ("K2", "fp32", (1, 64, 65, 64, 128, 3, 1, 1)),
    ("RING_64", "bf16", (1, 45, 46, 128, 128, 3, 1, 1)),
    ("PATCH_C64", "bf16", (1, 181, 182, 64, 64, 3, 1, 1)),
    ("TILED_128X64", "fp32", (1, 128, 129, 64, 64, 3, 1, 1)),
]
# where a kind has a threshold, the map one step smaller must plan to another kind (that is what "smallest" means)
DGRAD_KIND_THRESHOLDED = {"K2", "RING_64", "PATCH_C64", "TILED_128X64"}


def dgrad_ref(g, w, pad, dil, dtype):
    """float64 data gradient of a stride-1 conv from its pre-activation gradient g [N,Cout,Ho,Wo] (in the dtype) and weights w
    [Cout,Cin,k,k]: conv_transpose, with its magnitude; -> (dx, bound = 4 eps32 sqrt(k k Cout) mag + 1e-6 (+ h16 |dx|))"""
    gq, wq = q(g, dtype), q(w, dtype)
    dx = F.conv_transpose2d(gq, wq, None, 1, pad, 0, 1, dil)
    mag = F.conv_transpose2d(gq.abs(), wq.abs(), None, 1, pad, 0, 1, dil)
    k, cout = w.shape[2], w.shape[0]
    return dx, acc_bound(k * k * cout, mag) + e_store(dtype) * dx.abs()
