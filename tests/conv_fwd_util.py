"""Case table, inputs, float64 references and the two checks that test_conv_fwd_gpu.py holds every forward conv kernel to
(conv_fwd_plan of csrc/conv.hip picks among eleven), with a plain torch emulation of the device arithmetic that
test_conv_fwd_cpu.py plants faults into.  CPU and torch only; bounds and helpers come from trunk_bwd_util.py.

Two inputs per case:
  general   x ~ N(0,1), He-scaled w, scale 0.5 + rand, bias 0.1 randn, shortcut randn; operands rounded to their storage dtype, then a
            float64 reference conv * scale + bias (+ res * res_mult) -> ReLU.  Every output element must lie inside
            acc_bound(Cin k k, mag |scale|) + e_store(out dtype) |ref|   (mag: the same conv on |x|, |w|; ReLU is 1-Lipschitz, so
            the pre-activation bound carries over).
  grid      x multiples of 1/4 in [-2, 2], w multiples of 1/8 in [-1, 1], scale from {0.5, 1, 2}, bias and shortcut multiples of
            1/4 in [-4, 4], res_mult from {1, 0.5}.  Every product is a multiple of 2^-5 and with L <= 4608 every partial sum, in any
            order, stays below 2^14: fp32 accumulation and the epilogue are exact whatever the slab, k-step or wave order, and the
            only rounding is the final store.  Expected: float64 reference -> float32 -> out dtype, compared bit for bit.  The grid
            produces genuine ties, so this pins round-to-nearest-even at the store.
  grid8     the grid with scale from {1/8, 1/4, 1/2}, which keeps |y| <= 448 for the fp8 e4m3fn output of the fp8 recipe's stem.
"""
import collections
import functools
import math

import torch
import torch.nn.functional as F

from trunk_bwd_util import BF16, F32, KIND_NAMES, cin_pad, conv_fwd_ref, dname, e_store, out_hw, q, worst_ratio

FP8 = torch.float8_e4m3fn
FP8_MAX = 448.0
CUS = 256  # compute units of the MI355X: the CPU plan table is queried for this device
BF16_ONLY_KINDS = ("PATCH_C64", "PP256", "PP8", "PP8_WIDE", "RING_64", "RING_128")

# ---- shapes (N, H, W, Cin, Cout, k, stride, pad, dil) ------------------------------------------------------------------------------
A = (2, 9, 15, 64, 136, 3, 1, 2, 2)     # M = 270 = 2 x 128 + 14 = 256 + 14, an image boundary inside a tile, Cout = 128 + 8, 9 slabs, dilation-2 padding at every border
B = (1, 13, 11, 64, 72, 1, 1, 0, 1)     # one slab (fewer than any ring depth), M = 143, Cout = 64 + 8
C = (2, 17, 15, 128, 40, 3, 2, 1, 1)    # stride 2 on odd sizes, 18 slabs, Cout < 64
D = (2, 13, 11, 192, 264, 1, 1, 0, 1)   # 3 slabs, M = 286 = 256 + 30, Cout = 256 + 8
PP256_WIDE_N = (1, 17, 16, 64, 520, 1, 1, 0, 1)   # one slab, 2 x 3 tiles of 256 x 256, ragged both ways
PATCH = (2, 9, 35, 64, 64, 3, 1, 1, 1)            # 8 x 32-pixel blocks ragged in both directions
KS_RES4 = (1, 14, 14, 256, 256, 3, 1, 1, 1)
KS_SCALAR = (1, 9, 9, 512, 100, 1, 1, 0, 1)       # Cout % 8 != 0: the scalar epilogue
K2_1X1 = (1, 33, 31, 512, 328, 1, 1, 0, 1)        # M = 15 x 64 + 63, Cout = 5 x 64 + 8
K2_3X3 = (1, 33, 31, 128, 328, 3, 1, 2, 2)
STEM = (1, 21, 19, 3, 8, 3, 2, 1, 1)              # 3 channels stored as cin_pad(dtype)
T128X64 = (1, 128, 129, 16, 40, 3, 1, 1, 1)       # the threshold: the 127 x 128 map plans to TILED_64
T128 = (1, 65, 63, 16, 520, 3, 1, 1, 1)           # M = 31 x 128 + 127, Cout = 4 x 128 + 8

# ---- epilogue forms: name -> (scale, shortcut, relu) -------------------------------------------------------------------------------
FORMS = collections.OrderedDict([
    ("bn_relu", (True, False, True)),        # FrozenBN affine + ReLU
    ("bn_res", (True, True, False)),         # affine + shortcut, no ReLU
    ("bn_res_relu", (True, True, True)),     # affine + shortcut + ReLU
    ("vgg_relu", (False, False, True)),      # scale = None, bias, ReLU
])
SHORTCUT_FORMS = ("bn_res", "bn_res_relu")

# One case: the kernel it claims, a shape, the operands' dtype, the knobs (names of ops.TUNE_*) it is pinned with, and the storage
# of the output / shortcut (None: the operands' dtype).  res_mult None: 1 on general input, drawn from {1, 0.5} on the grid.
Case = collections.namedtuple("Case", "kind tag shape dtype knobs out_dtype res_dtype res_mult inputs forms")


def _case(kind, tag, shape, dtype=BF16, knobs=None, out_dtype=None, res_dtype=None, res_mult=None, inputs=("general", "grid"),
          forms=tuple(FORMS)):
    return Case(kind, tag, shape, dtype, tuple((knobs or {}).items()), out_dtype or dtype, res_dtype or dtype, res_mult, inputs, forms)


def _cases():
    out = []
    ad = (("A", A), ("B", B), ("C", C), ("D", D))
    # the pinned bf16 families.  TUNE_PP8_STAGES 3 / 4 / 5: the ring depth falls below, at and above the slab counts 1 / 3 / 9.
    # The three-stage ring is compiled for schedule variant 0 alone (any other pair of the two knobs runs five stages), so that row
    # pins the variant too; 4 and 5 stages run the shipped variant.
    for stages in (3, 4, 5):
        knobs = {"TUNE_PP8": 2, "TUNE_PP8_WIDE": 0, "TUNE_PP8_STAGES": stages}
        if stages == 3:
            knobs["TUNE_PP8_VARIANT"] = 0
        out += [_case("PP8", "%s-stages%d" % (n, stages), s, knobs=knobs) for n, s in ad]
    out += [_case("PP8_WIDE", n, s, knobs={"TUNE_PP8": 2, "TUNE_PP8_WIDE": 2}) for n, s in ad]
    out += [_case("RING_64", n, s, knobs={"TUNE_PP8": 0, "TUNE_CONV_RING": 64}) for n, s in ad]
    out += [_case("RING_128", n, s, knobs={"TUNE_PP8": 0, "TUNE_CONV_RING": 128}) for n, s in ad]
    out += [_case("PP256", n, s, knobs={"TUNE_CONV_PP": 2}) for n, s in (("D", D), ("wide_n", PP256_WIDE_N))]
    out.append(_case("PATCH_C64", "ragged", PATCH, knobs={"TUNE_CONV_PATCH": 2}))  # (2: the kernel on, from maps of 2 pixels)
    # the default-rule kinds, fp32 and bf16
    t64 = {"TUNE_CONV_K2_TILES": 0, "TUNE_CONV_KSPLIT": 0}
    for dtype in (F32, BF16):
        out += [_case("KS", n, s, dtype) for n, s in (("res4", KS_RES4), ("A", A), ("scalar_epilogue", KS_SCALAR))]
        out += [_case("K2", n, s, dtype) for n, s in (("1x1", K2_1X1), ("3x3_dil2", K2_3X3))]
        out += [_case("TILED_64", "A", A, dtype, t64), _case("TILED_64", "D", D, dtype, t64), _case("TILED_64", "stem", STEM, dtype)]
        out.append(_case("TILED_128X64", "threshold", T128X64, dtype))
        out.append(_case("TILED_128", "ragged", T128, dtype))
    # mixed storage (conv2d_nhwc_q), one KS and one TILED_64 shape each
    for kind, n, s, knobs in (("KS", "res4", KS_RES4, None), ("TILED_64", "A", A, t64)):
        out.append(_case(kind, n + "-out_fp32", s, BF16, knobs, out_dtype=F32))
        out.append(_case(kind, n + "-res_fp32_half", s, BF16, knobs, res_dtype=F32, res_mult=0.5, forms=SHORTCUT_FORMS))
        out.append(_case(kind, n + "-out_fp8", s, BF16, knobs, out_dtype=FP8, inputs=("grid8",)))
    return out


CASES = _cases()
CASE_FORMS = [(c, f) for c in CASES for f in c.forms]


def case_id(case):
    return "%s-%s-%s" % (case.kind, dname(case.dtype), case.tag)


def case_form_id(cf):
    return "%s-%s" % (case_id(cf[0]), cf[1])


def knob_dict(ops, case):
    """{ops.TUNE_*: value} in the case's order, for ops.tuned"""
    return collections.OrderedDict((getattr(ops, name), v) for name, v in case.knobs)


# ---- inputs -----------------------------------------------------------------------------------------------------------------------
def _seed(shape):
    return 7919 + sum((i + 1) * 131 ** (i % 3) * v for i, v in enumerate(shape))


@functools.lru_cache(maxsize=8)
def inputs(shape, dtype, kind):
    """float32 CPU tensors of one (shape, operand dtype, input kind): x [N,Cin,H,W] and w [Cout,Cin,k,k] as stored in `dtype`,
    scale / bias [Cout], the shortcut res [N,Cout,Ho,Wo] NOT yet rounded to its storage, and the grid's own res_mult"""
    n, h, w_, cin, cout, k, stride, pad, dil = shape
    ho, wo = out_hw(h, w_, k, stride, pad, dil)
    g = torch.Generator().manual_seed(_seed(shape) + (0 if kind == "general" else 1))
    if kind == "general":
        x = torch.randn((n, cin, h, w_), generator=g)
        wt = torch.randn((cout, cin, k, k), generator=g) * math.sqrt(2.0 / (cin * k * k))
        scale = 0.5 + torch.rand((cout,), generator=g)
        bias = torch.randn((cout,), generator=g) * 0.1
        res = torch.randn((n, cout, ho, wo), generator=g)
        res_mult = 1.0
    else:
        assert kind in ("grid", "grid8")
        ri = lambda shp, lo, hi: torch.randint(lo, hi + 1, shp, generator=g).float()
        x = ri((n, cin, h, w_), -8, 8) / 4
        wt = ri((cout, cin, k, k), -8, 8) / 8
        scales = torch.tensor([0.5, 1.0, 2.0] if kind == "grid" else [0.125, 0.25, 0.5])
        scale = scales[torch.randint(0, 3, (cout,), generator=g)]
        bias = ri((cout,), -16, 16) / 4
        res = ri((n, cout, ho, wo), -16, 16) / 4
        res_mult = (1.0, 0.5)[int(torch.randint(0, 2, (1,), generator=g))]
    x, wt = x.to(dtype).float(), wt.to(dtype).float()
    return dict(x=x, w=wt, scale=scale, bias=bias, res=res, res_mult=res_mult, ho=ho, wo=wo)


def res_mult_of(case, kind):
    return case.res_mult if case.res_mult is not None else inputs(case.shape, case.dtype, kind)["res_mult"]


# ---- the float64 reference ----------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=8)
def _affine_ref(shape, dtype, kind, with_scale):
    """(float64 conv * scale + bias, the accumulation bound acc_bound(Cin k k, mag |scale|)) of the stored operands: shared by every
    form, output storage and kernel that runs this (shape, dtype, input)"""
    p = inputs(shape, dtype, kind)
    stride, pad, dil = shape[6:]
    # the operands already hold their stored values, so conv_fwd_ref is asked for no further rounding and no storage term (F32)
    return conv_fwd_ref(p["x"], p["w"], p["scale"] if with_scale else None, p["bias"], None, stride, pad, dil, F32)


def reference(case, form, kind):
    """-> (float64 reference output [N,Cout,Ho,Wo] with the ReLU applied, per-element bound of the general-input check)"""
    with_scale, with_res, relu = FORMS[form]
    pre, acc = _affine_ref(case.shape, case.dtype, kind, with_scale)
    if with_res:
        pre = pre + q(inputs(case.shape, case.dtype, kind)["res"], case.res_dtype) * res_mult_of(case, kind)
    bound = acc + (e_store(case.out_dtype) if case.out_dtype != FP8 else float("nan")) * pre.abs()
    return (torch.relu(pre) if relu else pre), bound


def stored(ref, out_dtype):
    """what an exact epilogue stores: float64 -> float32 (exact on the grid) -> out dtype, round to nearest even"""
    return ref.float().to(out_dtype)


def same_bits(got, want):
    """bit for bit: torch.equal on bf16 / fp32, equal bytes on fp8"""
    assert got.dtype == want.dtype and got.shape == want.shape, (got.dtype, want.dtype, got.shape, want.shape)
    if got.dtype == FP8:
        return torch.equal(got.view(torch.uint8), want.view(torch.uint8))
    return torch.equal(got, want)


def general_ratio(got, ref, bound):
    """worst |got - ref| / bound over EVERY output element (<= 1 passes)"""
    return worst_ratio(got, ref, bound)


def grid_mismatches(got, ref, out_dtype):
    """[(index, got, want)] of the first few elements where the device differs from the stored exact result"""
    want = stored(ref, out_dtype)
    if same_bits(got, want):
        return []
    bad = (got.float() != want.float()).nonzero()
    return [(tuple(i.tolist()), float(got.float()[tuple(i)]), float(want.float()[tuple(i)])) for i in bad[:8]] + [("count", int(len(bad)))]


# ---- device layouts (built on the CPU; the GPU test moves them) ---------------------------------------------------------------------
def nhwc(t_nchw, dtype, cpad=None):
    n, c, h, w = t_nchw.shape
    out = torch.zeros((n, h, w, cpad or c), dtype=dtype)
    out[..., :c] = t_nchw.permute(0, 2, 3, 1).to(dtype)
    return out


def nchw(t_nhwc):
    return t_nhwc.permute(0, 3, 1, 2)


def pack_w(wt, dtype, cpad, kpad):
    """[Cout,Cin,k,k] -> [Cout, kpad(k k cpad)] with column (kh * k + kw) * cpad + ci, zero padded"""
    cout, cin, kh, kw = wt.shape
    wp = torch.zeros((cout, kh, kw, cpad))
    wp[..., :cin] = wt.permute(0, 2, 3, 1)
    out = torch.zeros((cout, kpad(kh * kw * cpad, dtype)), dtype=dtype)
    out[:, :kh * kw * cpad] = wp.reshape(cout, -1).to(dtype)
    return out


def call_args(ops, case, form, kind, device=None, shape=None):
    """the arguments of ops.conv2d_nhwc_q / ops.conv2d_plan for one (case, form, input): (x, w_packed, cout, k, k, stride, pad, dil,
    scale, bias, out_dtype, residual, res_mult, relu).  kind None: empty tensors of the right shapes (the host-only plan query);
    `shape` replaces the case's own (the plan query one step below a threshold)."""
    shape = shape or case.shape
    n, h, w_, cin, cout, k, stride, pad, dil = shape
    with_scale, with_res, relu = FORMS[form]
    cp = cin_pad(cin, case.dtype)
    ho, wo = out_hw(h, w_, k, stride, pad, dil)
    if kind is None:
        x = torch.empty((n, h, w_, cp), dtype=case.dtype)
        wp = torch.empty((cout, ops.kpad(k * k * cp, case.dtype)), dtype=case.dtype)
        scale, bias = torch.empty(cout), torch.empty(cout)
        res, res_mult = torch.empty((n, ho, wo, cout), dtype=case.res_dtype), case.res_mult or 1.0
    else:
        p = inputs(shape, case.dtype, kind)
        x, wp = nhwc(p["x"], case.dtype, cp), pack_w(p["w"], case.dtype, cp, ops.kpad)
        scale, bias = p["scale"].clone(), p["bias"].clone()
        res, res_mult = nhwc(p["res"], case.res_dtype), res_mult_of(case, kind)
    mv = (lambda t: t.to(device)) if device is not None else (lambda t: t)
    return (mv(x), mv(wp), cout, k, k, stride, pad, dil, mv(scale) if with_scale else None, mv(bias), case.out_dtype,
            mv(res) if with_res else None, res_mult if with_res else 1.0, relu)


def plan_name(ops, case, form, cus=CUS, shape=None):
    """the kernel conv_fwd_plan picks for the case under the knobs AS THEY STAND, queried host-only on CPU tensors"""
    return KIND_NAMES[ops.conv2d_plan(*call_args(ops, case, form, None, shape=shape), cus=cus)]


# ---- the device arithmetic in plain torch, with the faults the checks must see ------------------------------------------------------
FAULTS = ("trunc_store", "bf16_scale", "double_round", "missing_product", "missing_tap_channels")


def _bf16_truncate(y):
    return (y.contiguous().view(torch.int32) & -65536).view(torch.float32)


def emulate(case, form, kind, fault=None):
    """An fp32 conv of the stored operands, the affine, the shortcut, the ReLU and ONE store to the output dtype - what every kernel
    computes up to summation order - as the stored [N,Cout,Ho,Wo] tensor of the output dtype.  `fault` plants one of FAULTS:
      trunc_store           the bf16 store truncates instead of rounding to nearest even
      bf16_scale            the folded BN scale is rounded to bf16
      double_round          conv * scale + bias is rounded to bf16 before the shortcut is added
      missing_product       the last output pixel never reads the last channel of its centre tap: one product short per element
      missing_tap_channels  the last output row never reads the last 8 input channels of tap (0, 0)"""
    assert fault is None or fault in FAULTS
    n, h, w_, cin, cout, k, stride, pad, dil = case.shape
    with_scale, with_res, relu = FORMS[form]
    p = inputs(case.shape, case.dtype, kind)
    x, wt = p["x"], p["w"]
    y = F.conv2d(x, wt, None, stride, pad, dil)
    if fault == "missing_product":
        hi, wi = (p["ho"] - 1) * stride + (k // 2) * dil - pad, (p["wo"] - 1) * stride + (k // 2) * dil - pad
        assert 0 <= hi < h and 0 <= wi < w_
        y[-1, :, -1, -1] -= x[-1, cin - 1, hi, wi] * wt[:, cin - 1, k // 2, k // 2]
    if fault == "missing_tap_channels":
        assert 0 <= (p["ho"] - 1) * stride - pad < h and cin >= 8
        w2 = torch.zeros_like(wt)
        w2[:, -8:, 0, 0] = wt[:, -8:, 0, 0]
        y[:, :, -1, :] -= F.conv2d(x, w2, None, stride, pad, dil)[:, :, -1, :]
    if with_scale:
        scale = p["scale"].to(BF16).float() if fault == "bf16_scale" else p["scale"]
        y = y * scale.view(1, -1, 1, 1)
    y = y + p["bias"].view(1, -1, 1, 1)
    if fault == "double_round":
        y = y.to(BF16).float()
    if with_res:
        y = y + p["res"].to(case.res_dtype).float() * res_mult_of(case, kind)
    if relu:
        y = torch.relu(y)
    if fault == "trunc_store":
        assert case.out_dtype == BF16
        return _bf16_truncate(y).to(BF16)
    return y.to(case.out_dtype)
