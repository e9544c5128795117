"""Tensor-level wrappers over the C ABI (include/drn_wsod.h).  torch is used only to own device
memory and streams; every computation below is a hand-written HIP kernel.  No CPU path exists:
passing CPU tensors raises."""
import contextlib
import ctypes
import functools
import math

import numpy as np
import torch

from . import _cabi as C

SCALE_CLAMP = math.log(1000.0 / 16)  # detectron2/modeling/box_regression.py:9
GEMM_TIMING = None  # set to a list by bench.py to time GEMM launches with HIP events
HBM_TIMING = None   # likewise for the two HBM-bound kernels of the step (pooling launch, optimizer launches) - in-step figures


FP8 = torch.float8_e4m3fn  # OCP e4m3fn: gfx950's native fp8
FP8_MAX = 448.0


def esize(dtype):
    return 1 if dtype == FP8 else 2 if dtype == torch.bfloat16 else 4


def kpad(k, dtype):
    """K rounded up to a whole number of 128-byte slabs (GEMM contract)."""
    q = 128 // esize(dtype)
    return (k + q - 1) // q * q


def _2d(t):
    assert t.dim() == 2 and t.stride(1) == 1, "row-major 2-D tensor expected"
    return t.stride(0)


def gemm_set_tile(tile):
    """pin the GEMM tile (64/128/256; 0 = heuristic); returns the previous setting"""
    return C.lib().drn_gemm_set_tile(int(tile))


# the knob ids of include/drn_wsod.h (#define DRN_TUNE_*), by id; tests/test_tune_cpu.py holds the two lists equal
TUNE_GEMM_PERSISTENT = 1
TUNE_SGD_GRID = 2
TUNE_GEMM_GROUP_ROWS = 3
TUNE_ROI_MAP64 = 4
TUNE_CONV_KSPLIT = 5
TUNE_GEMM_TAIL_SPLIT = 6
TUNE_CONV_KS_TILES = 7
TUNE_CONV_K2_TILES = 8
TUNE_CONV_PATCH = 9
TUNE_ROI_CPB = 10
TUNE_ROI_PREFETCH = 11
TUNE_GEMM_PINGPONG = 12
TUNE_FP8_K64 = 13
TUNE_ROI_MAP64_A = 14
TUNE_ROI_LDS_KB = 15
TUNE_GEMM_NWG = 18
TUNE_ROI_LANE = 19
TUNE_SGDP_EPILOGUE = 20
TUNE_ROI_LANE_REPS = 22
TUNE_CONV_RING = 23
TUNE_CONV_PP = 24
TUNE_PP8 = 25
TUNE_PP8_STAGES = 26
TUNE_PP8_VARIANT = 27
TUNE_PP8_PROFILE = 28
TUNE_PP8_WIDE = 29
TUNE_PP8_WIDE_VARIANT = 30
TUNE_ROI_ST = 31
TUNE_MSM_WAVE = 32


def tune(knob, value):
    """drn_tune: set a tuning knob (A/B measurements, tests); returns the previous value"""
    return C.lib().drn_tune(int(knob), int(value))


@contextlib.contextmanager
def tuned(knobs=None, tile=None):
    """`with tuned({TUNE_PP8: 0, ...}) as prev:` sets the knobs in the dict's order, yields {knob: previous value} and on exit -
    an exception included - sets those previous values again, last knob first.  What is restored is what drn_tune returned,
    never a literal default.  `tile` pins the GEMM tile (gemm_set_tile) the same way; its previous value is prev["tile"]."""
    prev, undo = {}, []
    try:
        if tile is not None:
            prev["tile"] = gemm_set_tile(tile)
            undo.append((gemm_set_tile, prev["tile"]))
        for k, v in (knobs or {}).items():
            prev[k] = tune(k, v)
            undo.append((functools.partial(tune, k), prev[k]))
        yield prev
    finally:
        for fn, old in reversed(undo):
            fn(old)


def gemm_nt(A, B, M, N, K, out=None, splits=1, accumulate=False):
    """C[s,M,N] (fp32) = A[M,:K] @ B[N,:K]^T.  A, B: 2-D row-major device tensors of the compute dtype
    whose leading dimension may exceed K (zero padded up to kpad)."""
    lda, ldb = _2d(A), _2d(B)
    assert A.dtype == B.dtype
    if out is None:
        out = torch.empty((splits, M, N), dtype=torch.float32, device=A.device)
    assert out.dtype == torch.float32 or (out.dtype == torch.bfloat16 and splits == 1 and not accumulate)
    ldc = out.stride(-2)
    sstride = out.stride(0) if out.dim() == 3 else 0
    assert out.dim() == 3 or splits == 1
    if GEMM_TIMING is not None:  # bench.py: HIP events on the launching stream around this launch
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
    C.call("drn_gemm_nt", C.ptr(A), C.ptr(B), C.ptr(out), M, N, K, lda, ldb, ldc, C.dt(A.dtype), C.dt(out.dtype), splits,
           sstride, int(accumulate), C.stream())
    if GEMM_TIMING is not None:
        e1.record()
        GEMM_TIMING.append((e0, e1, 2.0 * M * N * K, (M, N, K)))
    return out


def gemm_nt_pair(g0, g1):
    """two independent gemm_nt problems in one persistent launch (drn_gemm_nt_pair); g = dict(A, B, M, N, K, out,
    splits=1, accumulate=False) with fp32 `out` [splits, M, N]"""
    args = []
    for g in (g0, g1):
        A, B, out = g["A"], g["B"], g["out"]
        assert A.dtype == torch.bfloat16 and B.dtype == torch.bfloat16 and out.dtype == torch.float32 and out.dim() == 3
        s_ = int(g.get("splits", 1))
        args += [C.ptr(A), C.ptr(B), C.ptr(out), int(g["M"]), int(g["N"]), int(g["K"]), _2d(A), _2d(B), out.stride(-2), s_,
                 out.stride(0), int(bool(g.get("accumulate", False)))]
    if GEMM_TIMING is not None:
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
    C.call("drn_gemm_nt_pair", *args, C.stream())
    if GEMM_TIMING is not None:
        e1.record()
        GEMM_TIMING.append((e0, e1, 2.0 * (g0["M"] * g0["N"] * g0["K"] + g1["M"] * g1["N"] * g1["K"]), ("pair",)))


def gemm_tn(A, Bt, M, N, K, kb_rows, out=None, splits=1, accumulate=False):
    """C[s,M,N] = A[M,:K] @ Bt[:K,:N] with the second operand K-major (Bt [kb_rows, ldb] row-major; rows kb_rows..K-1
    count as zeros and need not exist): drn_gemm_tn, bf16 operands.  The fc6 weight gradient reads the pooled matrix
    through it, so no transposed copy of it is written."""
    assert A.dtype == torch.bfloat16 and Bt.dtype == torch.bfloat16 and Bt.shape[0] >= kb_rows
    lda, ldb = _2d(A), _2d(Bt)
    if out is None:
        out = torch.empty((splits, M, N), dtype=torch.float32, device=A.device)
    assert out.dtype == torch.float32 or (out.dtype == torch.bfloat16 and splits == 1 and not accumulate)
    ldc = out.stride(-2)
    sstride = out.stride(0) if out.dim() == 3 else 0
    assert out.dim() == 3 or splits == 1
    if GEMM_TIMING is not None:
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
    C.call("drn_gemm_tn", C.ptr(A), C.ptr(Bt), C.ptr(out), M, N, K, int(kb_rows), lda, ldb, ldc, C.dt(out.dtype), splits,
           sstride, int(accumulate), C.stream())
    if GEMM_TIMING is not None:
        e1.record()
        GEMM_TIMING.append((e0, e1, 2.0 * M * N * K, (M, N, K)))
    return out


def gemm_tn_sgd(A, Bt, M, N, K, kb_rows, bucket, weights, mom, shadow, seg_dev, momentum, first_step, grad_scale=1.0,
                guard=None):
    """drn_gemm_tn_sgd: bucket[M, N] (bf16) = A[M,:K] @ Bt[:K,:N] and, in the same launch, the SGD step of weights[M, N] /
    mom / shadow (2-D views with a common row pitch) with that gradient.  Returns False when the shape is outside the
    kernel's class (nothing was launched: run gemm_tn + sgd_step_block instead).  guard: the int32 state of loss_guard()
    (drn_gemm_tn_sgd_guard: a set flag leaves weights / mom / shadow bit-unchanged); None = the unguarded entry point."""
    assert A.dtype == torch.bfloat16 and Bt.dtype == torch.bfloat16 and bucket.dtype == torch.bfloat16
    assert weights.dtype == torch.float32 and mom.dtype == torch.float32 and shadow.dtype == torch.bfloat16
    assert _2d(weights) == _2d(mom) == _2d(shadow)
    if GEMM_TIMING is not None:
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
    args = (C.ptr(A), C.ptr(Bt), C.ptr(bucket), M, N, K, int(kb_rows), _2d(A), _2d(Bt), _2d(bucket), C.ptr(weights),
            C.ptr(mom), C.ptr(shadow), _2d(weights), C.ptr(seg_dev), float(momentum), int(bool(first_step)), float(grad_scale))
    if guard is None:
        rc = C.lib().drn_gemm_tn_sgd(*args, C.stream())
    else:
        rc = C.lib().drn_gemm_tn_sgd_guard(*args, _guard_ptr(guard), C.stream())
    if rc == -3:
        return False
    if rc != 0:
        raise C.DrnError("drn_gemm_tn_sgd failed (%d)" % rc)
    if GEMM_TIMING is not None:
        e1.record()
        GEMM_TIMING.append((e0, e1, 2.0 * M * N * K, ("tn_sgd", M, N, K)))
    return True


def gemm_tn_acc_sgd(A, Bt, M, N, K, kb_rows, grad_acc, bucket, weights, mom, shadow, seg_dev, momentum, first_step,
                    grad_scale=1.0, guard=None):
    """drn_gemm_tn_acc_sgd: gemm_tn_sgd with bucket = bf16(grad_acc + A @ Bt) - the closing micro-step of a gradient-accumulation
    window; grad_acc [M, N] fp32 (a 2-D view, read only).  Returns False outside the kernel's shape class (nothing was launched:
    run gemm_tn(accumulate=True) + cast2d + sgd_step_block instead).  guard as in gemm_tn_sgd (drn_gemm_tn_acc_sgd_guard)."""
    assert A.dtype == torch.bfloat16 and Bt.dtype == torch.bfloat16 and bucket.dtype == torch.bfloat16
    assert grad_acc.dtype == torch.float32 and grad_acc.dim() == 2 and grad_acc.stride(1) == 1
    assert weights.dtype == torch.float32 and mom.dtype == torch.float32 and shadow.dtype == torch.bfloat16
    assert _2d(weights) == _2d(mom) == _2d(shadow)
    if GEMM_TIMING is not None:
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
    args = (C.ptr(A), C.ptr(Bt), C.ptr(grad_acc), C.ptr(bucket), M, N, K, int(kb_rows), _2d(A), _2d(Bt), _2d(grad_acc),
            _2d(bucket), C.ptr(weights), C.ptr(mom), C.ptr(shadow), _2d(weights), C.ptr(seg_dev), float(momentum),
            int(bool(first_step)), float(grad_scale))
    if guard is None:
        rc = C.lib().drn_gemm_tn_acc_sgd(*args, C.stream())
    else:
        rc = C.lib().drn_gemm_tn_acc_sgd_guard(*args, _guard_ptr(guard), C.stream())
    if rc == -3:
        return False
    if rc != 0:
        raise C.DrnError("drn_gemm_tn_acc_sgd failed (%d)" % rc)
    if GEMM_TIMING is not None:
        e1.record()
        GEMM_TIMING.append((e0, e1, 2.0 * M * N * K, ("tn_acc_sgd", M, N, K)))
    return True


def stage_heads_inputs(rois, props, words_src=None, words_dst=None):
    """props[M,4] <- rois[M,1:5]; words_dst <- words_src (int32 blocks of equal length), one launch"""
    assert rois.dtype == torch.float32 and props.dtype == torch.float32 and rois.is_contiguous() and props.is_contiguous()
    assert rois.shape[1] == 5 and props.shape == (rois.shape[0], 4)
    n = 0
    if words_src is not None:
        assert words_src.dtype == torch.int32 and words_dst.dtype == torch.int32 and words_src.numel() == words_dst.numel()
        n = words_src.numel()
    C.call("drn_stage_heads_inputs", C.ptr(rois), C.ptr(props), rois.shape[0], C.ptr(words_src), C.ptr(words_dst), n,
           C.stream())


def gemm_nt_main_cols(M, N, splits=1):
    """columns [0, n0) that drn_gemm_nt keeps for its persistent launch (n0 == N: no tail balancing for this shape)"""
    fn = C.lib().drn_gemm_nt_main_cols
    return int(fn(int(M), int(N), int(splits)))


def conv2d_nhwc(x, w_packed, cout, kh, kw, stride=1, pad=0, dil=1, scale=None, bias=None, residual=None, relu=False):
    """x [N,H,W,Cin] NHWC contiguous; w_packed [Cout, ldw]; returns y [N,Ho,Wo,Cout]."""
    assert x.is_contiguous() and x.dim() == 4
    n, h, w, cin = x.shape
    ho = (h + 2 * pad - dil * (kh - 1) - 1) // stride + 1
    wo = (w + 2 * pad - dil * (kw - 1) - 1) // stride + 1
    y = torch.empty((n, ho, wo, cout), dtype=x.dtype, device=x.device)
    if residual is not None:
        assert residual.shape == y.shape and residual.is_contiguous()
    C.call("drn_conv2d_nhwc", C.ptr(x), C.ptr(w_packed), C.ptr(y), C.ptr(scale), C.ptr(bias), C.ptr(residual), n, h, w,
           cin, cout, kh, kw, stride, pad, dil, _2d(w_packed), cout, cout, int(relu), C.dt(x.dtype), C.stream())
    return y


def conv2d_nhwc_q(x, w_packed, cout, kh, kw, stride, pad, dil, scale, bias, out_dtype, residual=None, res_mult=1.0,
                  relu=False):
    """drn_conv2d_nhwc_q: x / w_packed in one element type (fp32, bf16 or fp8 e4m3fn), y stored as out_dtype, an
    optional residual of any of the three types multiplied by res_mult before the add (see include/drn_wsod.h for how
    the quantisation scales enter `scale`, `bias` and `res_mult`)."""
    assert x.is_contiguous() and x.dim() == 4 and x.dtype == w_packed.dtype
    n, h, w, cin = x.shape
    ho = (h + 2 * pad - dil * (kh - 1) - 1) // stride + 1
    wo = (w + 2 * pad - dil * (kw - 1) - 1) // stride + 1
    y = torch.empty((n, ho, wo, cout), dtype=out_dtype, device=x.device)
    if residual is not None:
        assert residual.shape == y.shape and residual.is_contiguous()
    C.call("drn_conv2d_nhwc_q", C.ptr(x), C.ptr(w_packed), C.ptr(y), C.ptr(scale), C.ptr(bias), C.ptr(residual), n, h, w,
           cin, cout, kh, kw, stride, pad, dil, _2d(w_packed), cout, cout, int(relu), C.dt(x.dtype), C.dt(out_dtype),
           C.dt(residual.dtype) if residual is not None else 0, float(res_mult), C.stream())
    return y


# the kernel codes of drn_conv2d_plan (#define DRN_CONV_KIND_* of include/drn_wsod.h; tests/test_conv_plan_cpu.py holds them equal)
CONV_KIND_PATCH_C64 = 1
CONV_KIND_PP256 = 2
CONV_KIND_PP8 = 3
CONV_KIND_PP8_WIDE = 4
CONV_KIND_RING_64 = 5
CONV_KIND_RING_128 = 6
CONV_KIND_K2 = 7
CONV_KIND_KS = 8
CONV_KIND_TILED_64 = 9
CONV_KIND_TILED_128X64 = 10
CONV_KIND_TILED_128 = 11
CONV_KIND_FP8_K16 = 0x100
CONV_KINDS_TILED = (CONV_KIND_TILED_64, CONV_KIND_TILED_128X64, CONV_KIND_TILED_128)


def conv2d_plan(x, w_packed, cout, kh, kw, stride, pad, dil, scale, bias, out_dtype, residual=None, res_mult=1.0,
                relu=False, cus=0):
    """drn_conv2d_plan: the kernel (CONV_KIND_*, CONV_KIND_FP8_K16 or-ed in for the K = 16 fp8 form) that conv2d_nhwc_q runs
    these arguments on under the knobs as they stand, on a device of `cus` compute units (0: this device's).  Host-only:
    nothing is launched, allocated or dereferenced, so the tensors may live anywhere."""
    assert x.is_contiguous() and x.dim() == 4 and x.dtype == w_packed.dtype
    n, h, w, cin = x.shape
    at = lambda t: None if t is None else t.data_ptr()
    y = 4096  # (the output conv2d_nhwc_q allocates: a fresh, aligned tensor)
    rc = C.lib().drn_conv2d_plan(at(x), at(w_packed), y, at(scale), at(bias), at(residual), n, h, w, cin, cout, kh, kw, stride, pad,
                                 dil, _2d(w_packed), cout, cout, int(relu), C.dt(x.dtype), C.dt(out_dtype),
                                 C.dt(residual.dtype) if residual is not None else 0, float(res_mult), int(cus))
    if rc < 0:
        raise C.DrnError("drn_conv2d_plan failed: %s (%d)" % (C._ERR.get(rc, "error"), rc))
    return rc


def conv3x3_pw_nhwc(x, w2_packed, scale2, bias2, relu2, w3_packed=None, scale3=None, bias3=None, residual=None, res_mult=1.0,
                    relu3=True, pool=False, out=None):
    """drn_conv3x3_pw_nhwc: 3x3 (64 -> 64, pad 1) -> act [-> 1x1 (64 -> 256) + residual -> act] [-> 2x2 / stride-2 max pool] as
    one launch; x [N,H,W,64] bf16.  Returns y, or None when the shape is outside the kernel's class (run the separate ops)."""
    assert x.is_contiguous() and x.dim() == 4 and x.shape[3] == 64 and x.dtype == torch.bfloat16
    n, h, w, _ = x.shape
    cy = 256 if w3_packed is not None else 64
    ho, wo = ((h - 2) // 2 + 1, (w - 2) // 2 + 1) if pool else (h, w)
    y = out if out is not None else torch.empty((n, ho, wo, cy), dtype=x.dtype, device=x.device)
    if residual is not None:
        assert residual.shape == (n, h, w, cy) and residual.is_contiguous() and residual.dtype == x.dtype
    rc = C.lib().drn_conv3x3_pw_nhwc(C.ptr(x), C.ptr(w2_packed), C.ptr(scale2), C.ptr(bias2), int(relu2), C.ptr(w3_packed),
                                     C.ptr(scale3), C.ptr(bias3), C.ptr(residual), C.ptr(y), n, h, w, _2d(w2_packed),
                                     _2d(w3_packed) if w3_packed is not None else 0, float(res_mult), int(relu3), int(pool),
                                     C.stream())
    if rc == -3:
        return None
    if rc != 0:
        raise C.DrnError("drn_conv3x3_pw_nhwc failed (%d)" % rc)
    return y


def maxpool2x2_nhwc(x, stride):
    n, h, w, c = x.shape
    ho, wo = (h - 2) // stride + 1, (w - 2) // stride + 1
    y = torch.empty((n, ho, wo, c), dtype=x.dtype, device=x.device)
    C.call("drn_maxpool2x2_nhwc", C.ptr(x), C.ptr(y), n, h, w, c, stride, C.dt(x.dtype), C.stream())
    return y


def maxpool3x3s2_nhwc(x):
    """F.max_pool2d(x, kernel_size=3, stride=2, padding=1) on NHWC (the standard ResNet stem's pool)"""
    n, h, w, c = x.shape
    y = torch.empty((n, (h - 1) // 2 + 1, (w - 1) // 2 + 1, c), dtype=x.dtype, device=x.device)
    C.call("drn_maxpool3x3s2_nhwc", C.ptr(x), C.ptr(y), n, h, w, c, C.dt(x.dtype), C.stream())
    return y


def stem7x7_pool_nhwc(x, w_packed, cout, scale, bias, relu=True):
    """conv 7x7 / 2 / 3 + affine + ReLU + max_pool2d(3, 2, 1) as one launch (drn_stem7x7_pool_nhwc) -> the pooled map, or
    None where the shape is outside the kernel's class (the caller then runs conv2d_nhwc + maxpool3x3s2_nhwc)"""
    n, h, w, cin = x.shape
    ho, wo = (h - 1) // 2 + 1, (w - 1) // 2 + 1
    y = torch.empty((n, (ho - 1) // 2 + 1, (wo - 1) // 2 + 1, cout), dtype=x.dtype, device=x.device)
    rc = C.lib().drn_stem7x7_pool_nhwc(C.ptr(x), C.ptr(w_packed), C.ptr(scale), C.ptr(bias), C.ptr(y), n, h, w, cin, cout,
                                       w_packed.stride(0), int(bool(relu)), C.dt(x.dtype), C.stream())
    if rc == -3:
        return None
    if rc != 0:
        raise C.DrnError("drn_stem7x7_pool_nhwc failed (%d)" % rc)
    return y


def preprocess_nhwc(images, mean, std, dtype, cpad):
    """images: list of [3,H,W] f32 device tensors -> ([N,Hmax,Wmax,cpad] NHWC, sizes)."""
    hmax = max(int(i.shape[1]) for i in images)
    wmax = max(int(i.shape[2]) for i in images)
    out = torch.empty((len(images), hmax, wmax, cpad), dtype=dtype, device=images[0].device)
    m, s = C.host_floats(mean), C.host_floats(std)
    for k, im in enumerate(images):
        im = im.contiguous().float()
        C.call("drn_preprocess_nhwc", C.ptr(im), im.shape[0], im.shape[1], im.shape[2], C.ptr(out[k]), hmax, wmax, cpad,
               ctypes.cast(m, ctypes.c_void_p), ctypes.cast(s, ctypes.c_void_p), C.dt(dtype), C.stream())
    return out, [(int(i.shape[1]), int(i.shape[2])) for i in images]


def pil_bilinear_coeffs(in_size, out_size):
    """Pillow's resampling windows and 22-bit coefficients of a BILINEAR resize of `in_size` positions to `out_size`
    (Resample.c: precompute_coeffs + normalize_coeffs_8bpc), with Pillow's double arithmetic in Pillow's operation order:
    -> (bounds int32 [out, 2] = (first source position, count), coef int32 [out, ksize], ksize)"""
    import numpy as np

    scale = float(in_size) / out_size
    fscale = scale if scale >= 1.0 else 1.0
    support = 1.0 * fscale  # (the triangle filter's support is 1)
    ksize = int(math.ceil(support)) * 2 + 1
    ss = 1.0 / fscale
    center = 0.0 + (np.arange(out_size, dtype=np.float64) + 0.5) * scale
    xmin = np.maximum((center - support + 0.5).astype(np.int64), 0)  # (int) truncates, and the operands are > -1
    xmax = np.minimum((center + support + 0.5).astype(np.int64), in_size) - xmin
    kk = np.zeros((out_size, ksize), dtype=np.float64)
    ww = np.zeros(out_size, dtype=np.float64)
    for x in range(ksize):  # (column by column: the same summation order as Pillow's loop over x)
        a = np.abs(((x + xmin).astype(np.float64) - center + 0.5) * ss)
        w = np.where((a < 1.0) & (x < xmax), 1.0 - a, 0.0)
        kk[:, x] = w
        ww = ww + w
    nz = ww != 0.0
    kk[nz] = kk[nz] / ww[nz, None]
    coef = np.where(kk < 0, (-0.5 + kk * (1 << 22)).astype(np.int64), (0.5 + kk * (1 << 22)).astype(np.int64)).astype(np.int32)
    return np.stack([xmin, xmax], 1).astype(np.int32), coef, ksize


_RESIZE_COEFFS = {}


def _resize_tables(n_in, n_out, dev):
    """device copies of pil_bilinear_coeffs(n_in, n_out), cached: (bounds, coef, ksize); (None, None, 0) when the size stays"""
    if n_in == n_out:
        return None, None, 0
    key = (n_in, n_out, dev)
    t = _RESIZE_COEFFS.get(key)
    if t is None:
        if len(_RESIZE_COEFFS) > 256:
            _RESIZE_COEFFS.clear()
        b, k, ks = pil_bilinear_coeffs(n_in, n_out)
        t = _RESIZE_COEFFS[key] = (torch.from_numpy(b).to(dev), torch.from_numpy(k).to(dev), ks)
    return t


def resize_bilinear_u8(img_hwc, new_h, new_w, flip=False, out=None):
    """img_hwc: uint8 [H, W, C] device tensor -> fp32 [C, new_h, new_w] holding exactly the bytes
    PIL.Image.fromarray(img).resize((new_w, new_h), BILINEAR) produces (mirrored left-right when `flip`): ResizeTransform
    [+ HFlipTransform] of the TTA mapper on the device (drn_resize_bilinear_u8)."""
    assert img_hwc.dtype == torch.uint8 and img_hwc.dim() == 3 and img_hwc.is_contiguous() and img_hwc.is_cuda
    h, w, c = img_hwc.shape
    dev = img_hwc.device
    xb, xk, ksx = _resize_tables(w, new_w, dev)
    yb, yk, ksy = _resize_tables(h, new_h, dev)
    if out is None:
        out = torch.empty((c, new_h, new_w), dtype=torch.float32, device=dev)
    C.call("drn_resize_bilinear_u8", C.ptr(img_hwc), h, w, c, C.ptr(out), new_h, new_w, C.ptr(xb), C.ptr(xk), ksx, C.ptr(yb),
           C.ptr(yk), ksy, int(bool(flip)), C.stream())
    return out


_HOST_COEFFS = {}


def pil_bilinear_coeffs_cached(n_in, n_out):
    """pil_bilinear_coeffs on the host, remembered (numpy arrays: nothing on the device) -> (bounds, coef, ksize)"""
    t = _HOST_COEFFS.get((n_in, n_out))
    if t is None:
        if len(_HOST_COEFFS) > 1024:
            _HOST_COEFFS.clear()
        t = _HOST_COEFFS[(n_in, n_out)] = pil_bilinear_coeffs(n_in, n_out)
    return t


def augment_u8(src, crop, out_hw, flip=False, wb=None, ws=None, out=None, tables=None):
    """The training DatasetMapper's image chain in one launch (drn_augment_u8).  src: uint8 [H, W, C] device tensor, C in
    {1, 3, 4}; crop = (x0, y0, cw, ch) inside the image (None: the whole image); out_hw = (Ho, Wo) of the Pillow BILINEAR resize of
    the crop; flip mirrors the columns; wb / ws are RandomBrightness' / RandomSaturation's drawn weights, None switches that
    blend off (ws needs C == 3).  tables = ((xbounds, xcoef, ksx), (ybounds, ycoef, ksy)), int32 device tensors of
    pil_bilinear_coeffs(cw, Wo) / (ch, Ho) with (None, None, 0) where the size stays, for a caller that uploads them itself (the
    device mapper: one pinned copy with the image); by default they come from the _RESIZE_COEFFS cache.
    -> fp32 [C, Ho, Wo] holding exactly the bytes the host chain CropTransform ->
    ResizeTransform -> HFlipTransform -> BlendTransform x 2 produces (the saturation's grey value summed in index order)."""
    assert src.dtype == torch.uint8 and src.dim() == 3 and src.is_contiguous() and src.is_cuda
    h, w, c = src.shape
    x0, y0, cw, ch = (0, 0, w, h) if crop is None else (int(v) for v in crop)
    ho, wo = int(out_hw[0]), int(out_hw[1])
    if cw <= 0 or ch <= 0 or x0 < 0 or y0 < 0 or x0 + cw > w or y0 + ch > h:
        raise C.DrnError("augment_u8: crop (%d, %d, %d, %d) is not inside the %d x %d image" % (x0, y0, cw, ch, w, h))
    dev = src.device
    if tables is None:
        xb, xk, ksx = _resize_tables(cw, wo, dev)
        yb, yk, ksy = _resize_tables(ch, ho, dev)
    else:
        (xb, xk, ksx), (yb, yk, ksy) = tables
        for b, k, ks, n_out in ((xb, xk, ksx, wo), (yb, yk, ksy, ho)):
            assert b is None or (b.dtype == k.dtype == torch.int32 and b.numel() == 2 * n_out and k.numel() == n_out * ks
                                 and b.is_contiguous() and k.is_contiguous())
    if out is None:
        out = torch.empty((c, ho, wo), dtype=torch.float32, device=dev)
    assert out.shape == (c, ho, wo) and out.dtype == torch.float32 and out.is_contiguous()
    C.call("drn_augment_u8", C.ptr(src), h, w, c, x0, y0, cw, ch, C.ptr(out), ho, wo, C.ptr(xb), C.ptr(xk), ksx, C.ptr(yb),
           C.ptr(yk), ksy, int(bool(flip)), int(wb is not None), 0.0 if wb is None else float(wb), int(ws is not None),
           0.0 if ws is None else 1 - float(ws), 0.0 if ws is None else float(ws), C.stream())
    return out


def augment_u8_lds_bytes(crop_wh, out_hw, c):
    """LDS staging bytes drn_augment_u8 asks for at these sizes; 0 = the launch runs its one-thread-per-pixel path (the source
    window of a 64 x 16 output tile does not fit: strong down-scaling).  Host arithmetic only."""
    cw, ch = int(crop_wh[0]), int(crop_wh[1])
    ho, wo = int(out_hw[0]), int(out_hw[1])
    n = C.lib().drn_augment_lds_bytes(cw, ch, ho, wo, int(c), int(cw != wo), int(ch != ho))
    if n < 0:
        raise C.DrnError("drn_augment_lds_bytes failed (%d)" % n)
    return int(n)


ROI_WORKSPACE = True  # tools / tests: False = pool without the chunk-major scratch copy (same results)


def roi_pool_nhwc(feat, rois, objectness, P, scale, mode=0, sampling_ratio=0, aligned=False, out=None, out_dtype=None,
                  want_argmax=False, out_t=None, t_first_channel=0):
    """feat [N,H,W,C]; rois [M,5] f32; -> out [M, ld] (first C*P*P columns valid, k = c*P*P + bin); out_t (optional,
    [C*P*P, ld_t]) receives the transposed copy in the same call - with t_first_channel > 0 only its rows from channel
    t_first_channel on are guaranteed (drn_roi_pool_nhwc_t)."""
    n, h, w, c = feat.shape
    m = rois.shape[0]
    out_dtype = out_dtype or feat.dtype
    if out is None:
        out = torch.zeros((m, kpad(c * P * P, out_dtype)), dtype=out_dtype, device=feat.device)
    arg = torch.empty((m, c * P * P), dtype=torch.int32, device=feat.device) if want_argmax else None
    if out_t is not None:
        assert out_t.dtype == out.dtype
    if HBM_TIMING is not None:  # bench.py: HIP events on the launching stream around this launch
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
    # scratch for the chunk-major copy of large maps (drn_roi_pool_nhwc_ws): from torch's caching allocator on the current stream,
    # nothing is kept between calls; 0 bytes for every shape whose kernel does not use one (the bench shape among them)
    ws_bytes = C.lib().drn_roi_pool_workspace_bytes(n, h, w, c, P, m, mode, int(want_argmax), C.dt(feat.dtype), C.dt(out.dtype))
    ws = torch.empty((ws_bytes,), dtype=torch.uint8, device=feat.device) if ws_bytes > 0 and ROI_WORKSPACE else None
    C.call("drn_roi_pool_nhwc_ws", C.ptr(feat), C.ptr(rois), C.ptr(objectness), C.ptr(out), C.ptr(out_t), C.ptr(arg), n, h,
           w, c, P, m, float(scale), _2d(out), _2d(out_t) if out_t is not None else 0, mode, sampling_ratio,
           int(aligned), C.dt(feat.dtype), C.dt(out.dtype), int(t_first_channel), C.ptr(ws), ws_bytes if ws is not None else 0,
           C.stream())
    if HBM_TIMING is not None:
        e1.record()
        es = esize(out.dtype)
        t_rows = 0 if out_t is None else (c - min(c, t_first_channel // 8 * 8)) * P * P  # rows of out_t really written
        nbytes = m * c * P * P * es + m * t_rows * es + feat.numel() * esize(feat.dtype) + rois.numel() * 4
        HBM_TIMING.append((e0, e1, nbytes, ("roi_pool", m, c * P * P, out_t is not None)))
    return (out, arg) if want_argmax else out


def stage_rois(boxes, logits, batch_index=0.0):
    """boxes [M, 4] f32 (+ logits [M] f32 or None) of ONE image -> (rois [M, 5], obj [M] or None, props [M, 4]) in one launch
    (drn_stage_rois: convert_boxes_to_pooler_format + the contiguous copies the heads read)"""
    assert boxes.is_cuda and boxes.dtype == torch.float32 and boxes.dim() == 2 and boxes.is_contiguous() and boxes.shape[1] == 4
    M = boxes.shape[0]
    rois = torch.empty((M, 5), dtype=torch.float32, device=boxes.device)
    props = torch.empty((M, 4), dtype=torch.float32, device=boxes.device)
    obj = None
    if logits is not None:
        assert (logits.is_cuda and logits.device == boxes.device and logits.dtype == torch.float32 and logits.dim() == 1 and
                logits.is_contiguous() and logits.shape[0] == M), "objectness logits: a contiguous f32 [M] tensor on the boxes' device"
        obj = torch.empty((M,), dtype=torch.float32, device=boxes.device)
    C.call("drn_stage_rois", C.ptr(boxes), C.ptr(logits), float(batch_index), C.ptr(rois), C.ptr(obj), C.ptr(props), M, C.stream())
    return rois, obj, props


def im2col_t(x, cin, kh, kw, stride, pad, dil, out=None):
    """x [N,H,W,Cpad] NHWC -> [cin*kh*kw, kpad(N*Ho*Wo)] (row (ci*kh + i)*kw + j), zero padded columns."""
    n, h, w, cp = x.shape
    ho = (h + 2 * pad - dil * (kh - 1) - 1) // stride + 1
    wo = (w + 2 * pad - dil * (kw - 1) - 1) // stride + 1
    if out is None:
        out = torch.zeros((cin * kh * kw, kpad(n * ho * wo, x.dtype)), dtype=x.dtype, device=x.device)
    C.call("drn_im2col_t", C.ptr(x), C.ptr(out), n, h, w, cin, cp, kh, kw, stride, pad, dil, _2d(out), C.dt(x.dtype),
           C.stream())
    return out


def maxpool2x2_bwd_nhwc(x, dy, stride):
    n, h, w, c = x.shape
    assert dy.dtype == x.dtype and dy.is_contiguous() and x.is_contiguous()
    dx = torch.empty_like(x)
    C.call("drn_maxpool2x2_bwd_nhwc", C.ptr(x), C.ptr(dy), C.ptr(dx), n, h, w, c, stride, C.dt(x.dtype), C.stream())
    return dx


def add(a, b, out=None):
    assert a.dtype == b.dtype and a.numel() == b.numel() and a.is_contiguous() and b.is_contiguous()
    if out is None:
        out = torch.empty_like(a)
    C.call("drn_add", C.ptr(a), C.ptr(b), C.ptr(out), a.numel(), C.dt(a.dtype), C.stream())
    return out


def roi_backward_det_ws_bytes(n, h, w, m):
    """bytes of workspace drn_roi_pool_backward_det_nhwc needs (host-only: no device is touched)"""
    return C.lib().drn_roi_backward_det_ws_bytes(int(n), int(h), int(w), int(m))


def roi_pool_backward_nhwc(grad_out, rois, objectness, feat_shape, P, scale, mode=0, sampling_ratio=0, aligned=False,
                           argmax=None, deterministic=None, out=None):
    """grad_out [M, >= C*P*P] -> d(feat) [N,H,W,C] fp32 (see drn_roi_pool_backward_nhwc).
    deterministic: True = the order-fixed, atomic-free form (drn_roi_pool_backward_det_nhwc: bit-reproducible, RoIPool
    bit-equal to a sequential host scatter), False = the atomic scatter, None = the package's mode (set_deterministic).
    out: an fp32 [N,H,W,C] tensor to write into (every element is written)."""
    from . import get_deterministic

    n, h, w, c = feat_shape
    m = rois.shape[0]
    assert grad_out.is_cuda and rois.is_cuda, "drn ops need device tensors (no CPU path)"
    if out is None:
        out = torch.empty((n, h, w, c), dtype=torch.float32, device=grad_out.device)
    dfeat = out
    assert dfeat.is_cuda and dfeat.dtype == torch.float32 and dfeat.is_contiguous() and tuple(dfeat.shape) == (n, h, w, c)
    if get_deterministic() if deterministic is None else deterministic:
        # scratch for the per-tile ROI lists: from torch's caching allocator on the current stream, nothing is kept between calls
        ws_bytes = roi_backward_det_ws_bytes(n, h, w, m)
        ws = torch.empty((ws_bytes,), dtype=torch.uint8, device=grad_out.device)
        C.call("drn_roi_pool_backward_det_nhwc", C.ptr(grad_out), C.ptr(rois), C.ptr(objectness), C.ptr(argmax), C.ptr(dfeat),
               n, h, w, c, P, m, float(scale), _2d(grad_out), mode, sampling_ratio, int(aligned), C.dt(grad_out.dtype),
               C.ptr(ws), ws_bytes, C.stream())
        return dfeat
    C.call("drn_roi_pool_backward_nhwc", C.ptr(grad_out), C.ptr(rois), C.ptr(objectness), C.ptr(argmax), C.ptr(dfeat),
           n, h, w, c, P, m, float(scale), _2d(grad_out), mode, sampling_ratio, int(aligned), C.dt(grad_out.dtype),
           C.stream())
    return dfeat


def transpose2d(inp, rows, cols, out=None, out_dtype=None):
    out_dtype = out_dtype or inp.dtype
    if out is None:
        out = torch.zeros((cols, kpad(rows, out_dtype)), dtype=out_dtype, device=inp.device)
    C.call("drn_transpose2d", C.ptr(inp), C.ptr(out), rows, cols, _2d(inp), _2d(out), C.dt(inp.dtype), C.dt(out.dtype),
           C.stream())
    return out


def cast2d(inp, rows, cols, out):
    C.call("drn_cast2d", C.ptr(inp), C.ptr(out), rows, cols, _2d(inp), _2d(out), C.dt(inp.dtype), C.dt(out.dtype),
           C.stream())
    return out


def counter_add(counter, inc=1):
    C.call("drn_counter_add", C.ptr(counter), int(inc), C.stream())


def bias_act_fwd(partials, M, N, bias=None, relu=True, mask=None, seed=0, drop_p=0.0, out=None, outT=None, seed_dev=None):
    splits = partials.shape[0] if partials.dim() == 3 else 1
    sstride = partials.stride(0) if partials.dim() == 3 else 0
    ref = out if out is not None else outT
    C.call("drn_bias_act_fwd", C.ptr(partials), splits, sstride, C.ptr(bias), C.ptr(mask), int(seed), C.ptr(seed_dev),
           float(drop_p),
           C.ptr(out), _2d(out) if out is not None else 0, C.ptr(outT), _2d(outT) if outT is not None else 0, M, N,
           partials.stride(-2), int(relu), C.dt(ref.dtype), C.stream())


def linear_act_fwd(A, W, M, N, K, bias=None, relu=True, mask=None, seed=0, drop_p=0.0, out=None, outT=None, seed_dev=None):
    """drn_linear_act_fwd: out [M, N] (bf16) = dropout(relu(A[M,:K] @ W[N,:K]^T + bias)) and optionally its transpose, ONE launch
    (no split-K partials, no second pass).  Returns False when the shape is outside the kernel's class (the caller then runs
    gemm_nt + bias_act_fwd)."""
    assert A.dtype == W.dtype == torch.bfloat16 and out is not None and out.dtype == torch.bfloat16
    rc = C.lib().drn_linear_act_fwd(C.ptr(A), C.ptr(W), C.ptr(bias), C.ptr(mask), int(seed), C.ptr(seed_dev), float(drop_p),
                                    C.ptr(out), _2d(out), C.ptr(outT), _2d(outT) if outT is not None else 0, M, N, K, _2d(A),
                                    _2d(W), int(relu), C.stream())
    if rc == -3:
        return False
    if rc != 0:
        raise C.DrnError("drn_linear_act_fwd failed (%d)" % rc)
    return True


def bias_act_bwd(grad_out, M, N, saved=None, mask=None, drop_p=0.0, colscale=None, dpre=None, dpreT=None, colsum=None,
                 accumulate_colsum=False, colpart=None, colidx=None):
    ref = dpre if dpre is not None else dpreT
    if saved is not None and dpre is not None:
        assert _2d(saved) == _2d(dpre)
    ld_out = _2d(dpre) if dpre is not None else (_2d(saved) if saved is not None else 0)
    if colsum is not None and colpart is None:
        colpart = torch.empty(((M + 63) // 64, N), dtype=torch.float32, device=grad_out.device)
    if grad_out.dim() == 3:  # [splits, M, ld]: fp32 split-K partials of the dX GEMM, summed on load
        C.call("drn_bias_act_bwd_splits", C.ptr(grad_out), C.dt(grad_out.dtype), grad_out.stride(-2), grad_out.shape[0],
               grad_out.stride(0), C.ptr(colscale), C.ptr(colidx), C.ptr(saved), C.ptr(mask), float(drop_p), C.ptr(dpre),
               ld_out, C.ptr(dpreT), _2d(dpreT) if dpreT is not None else 0, C.ptr(colsum), C.ptr(colpart),
               int(accumulate_colsum), M, N, C.dt(ref.dtype), C.stream())
        return
    C.call("drn_bias_act_bwd", C.ptr(grad_out), C.dt(grad_out.dtype), _2d(grad_out), C.ptr(colscale), C.ptr(colidx),
           C.ptr(saved), C.ptr(mask), float(drop_p),
           C.ptr(dpre), ld_out, C.ptr(dpreT), _2d(dpreT) if dpreT is not None else 0, C.ptr(colsum), C.ptr(colpart),
           int(accumulate_colsum), M, N, C.dt(ref.dtype), C.stream())


def gemm_nt_act_bwd(A, B, M, N, K, saved=None, mask=None, drop_p=0.0, dpre=None, dpreT=None, colsum=None,
                    accumulate_colsum=False, colpart=None):
    """drn_gemm_nt_act_bwd: bias_act_bwd of the product A . B^T without the product going to memory (skinny K, bf16).
    Returns False when the shape is outside the kernel's class (the caller then runs gemm_nt + bias_act_bwd)."""
    ref = dpre if dpre is not None else dpreT
    assert A.dtype == torch.bfloat16 and B.dtype == torch.bfloat16 and ref.dtype == torch.bfloat16
    if saved is not None and dpre is not None:
        assert _2d(saved) == _2d(dpre)
    ld_out = _2d(dpre) if dpre is not None else (_2d(saved) if saved is not None else 0)
    if colsum is not None and colpart is None:
        colpart = torch.empty(((M + 63) // 64, N), dtype=torch.float32, device=A.device)
    rc = C.lib().drn_gemm_nt_act_bwd(C.ptr(A), C.ptr(B), M, N, K, _2d(A), _2d(B), C.ptr(saved), C.ptr(mask), float(drop_p),
                                     C.ptr(dpre), ld_out, C.ptr(dpreT), _2d(dpreT) if dpreT is not None else 0,
                                     C.ptr(colsum), C.ptr(colpart), int(accumulate_colsum), C.stream())
    if rc == -3:
        return False
    if rc != 0:
        raise C.DrnError("drn_gemm_nt_act_bwd failed (%d)" % rc)
    return True


def colsum_reduce(colpart, nparts, N, colsum, accumulate=False):
    """finish the two-stage column sums that bias_act_bwd(colsum=None, colpart=...) left as per-block partials"""
    C.call("drn_colsum_reduce", C.ptr(colpart), int(nparts), int(N), C.ptr(colsum), int(accumulate), C.stream())


def wsddn_fwd_bwd(logits, c_cls, c_det, K, img_off, n_img, gt_onehot, dlogits=None, mean_loss=True, loss_scale=1.0,
                  max_rows=None, return_rowsm=False):
    M = logits.shape[0]
    max_rows = max_rows or M
    dev = logits.device
    scores = torch.empty((M, K), dtype=torch.float32, device=dev)
    img_scores = torch.empty((n_img, K), dtype=torch.float32, device=dev)
    loss_part = torch.empty((n_img,), dtype=torch.float32, device=dev)
    rowsm = torch.empty((M, K), dtype=torch.float32, device=dev)
    scratch = torch.empty((n_img * ((max_rows + 31) // 32) * 384,), dtype=torch.float32, device=dev)
    C.call("drn_wsddn_fwd_bwd", C.ptr(logits), _2d(logits), c_cls, c_det, K, C.ptr(img_off), n_img, C.ptr(gt_onehot),
           C.ptr(scores), C.ptr(rowsm), C.ptr(img_scores), C.ptr(loss_part), C.ptr(dlogits),
           _2d(dlogits) if dlogits is not None else 0, C.ptr(scratch), int(max_rows), int(mean_loss), float(loss_scale),
           C.stream())
    if return_rowsm:
        return scores, img_scores, loss_part, rowsm
    return scores, img_scores, loss_part


def csc_cpg(dimg_nhwc, n_colours, out=None):
    """drn_csc_cpg: d score / d image [1, H, W, Cpad] -> the normalised map [H, W] fp32 (roi_heads_csc.py:456-464)"""
    n, H, W, cp = dimg_nhwc.shape
    assert n == 1 and dimg_nhwc.is_contiguous()
    if out is None:
        out = torch.empty((H, W), dtype=torch.float32, device=dimg_nhwc.device)
    scratch = torch.empty((1,), dtype=torch.int32, device=dimg_nhwc.device)
    C.call("drn_csc_cpg", C.ptr(dimg_nhwc), C.dt(dimg_nhwc.dtype), cp, n_colours, H, W, C.ptr(out), C.ptr(scratch), C.stream())
    return out


def csc_weights(cpg, fg_threshold, rois5, scores, c, area_sqrt, context_scale, W_out, table=None):
    """drn_csc_weights: column c of the CSC weights W_out [M, K] from one class map (csc_cuda.cu:398-535)"""
    H, Wd = cpg.shape
    M, K = scores.shape
    assert cpg.is_contiguous() and rois5.is_contiguous() and scores.is_contiguous() and W_out.is_contiguous()
    if table is None:
        table = torch.empty((H, Wd), dtype=torch.float32, device=cpg.device)
    C.call("drn_csc_weights", C.ptr(cpg), H, Wd, float(fg_threshold), C.ptr(rois5), M, C.ptr(scores), K, int(c),
           int(area_sqrt), float(context_scale), C.ptr(table), C.ptr(W_out), C.stream())
    return W_out


def csc_loss(logits, c_cls, c_det, K, scores, rowsm, W, onehot, mean_loss, dlogits=None, seed_class=None):
    """drn_csc_loss.  seed_class None: the two CSC losses [2] (+ their dlogits); else d (sum_r s[r, seed_class]) / d logits"""
    M = scores.shape[0]
    mode = 0 if seed_class is None else 1
    loss = torch.empty((2,), dtype=torch.float32, device=scores.device) if mode == 0 else None
    C.call("drn_csc_loss", C.ptr(logits), _2d(logits), c_cls, c_det, K, M, C.ptr(scores), C.ptr(rowsm), C.ptr(W),
           C.ptr(onehot), mode, int(seed_class or 0), int(mean_loss), C.ptr(loss), C.ptr(dlogits),
           _2d(dlogits) if dlogits is not None else 0, C.stream())
    return loss


CSC_MAX_IMAGES, CSC_MAX_K = 16, 128  # include/drn_wsod.h DRN_CSC_MAX_IMAGES, the K limit of drn_csc_loss


def csc_batch_limits(n_img, K, sizes=None):
    """the limits of CSC on image batches (include/drn_wsod.h), refused on the host before any launch or upload"""
    if not 1 <= int(n_img) <= CSC_MAX_IMAGES:
        raise C.DrnError("CSC image batch: %d images, 1 .. %d are built" % (n_img, CSC_MAX_IMAGES))
    if not 1 <= int(K) <= CSC_MAX_K:
        raise C.DrnError("CSC image batch: K = %d classes, 1 .. %d are built" % (K, CSC_MAX_K))
    for H, W in sizes or ():
        if H < 1 or W < 1 or H * W >= 1 << 24:
            raise C.DrnError("CSC image batch: an image of %d x %d pixels; 1 .. 2^24 - 1 pixels keep the fp32 counts of the "
                             "summed-area table exact" % (H, W))


class CscBatchPlan:
    """What one CSC step on an image batch tells the device, as ONE int64 upload (the layout of include/drn_wsod.h, "CSC on
    image batches"): hw [n, 2] | map_off [n] | slots [S, n] | pairs [P, 2] | tab_off [P].  `sizes`: (H_i, W_i) per image;
    `slots`: S rows of n classes (-1 = none), `pairs`: every (image, labelled class).  Host copies stay for the wrappers:
    map_floats / table_floats are what `maps` / `tables` have to hold."""

    def __init__(self, sizes, K, slots, pairs, device):
        sizes = [(int(h), int(w)) for h, w in sizes]
        n = len(sizes)
        csc_batch_limits(n, K, sizes)
        slots = [[int(c) for c in row] for row in slots]
        pairs = [(int(i), int(c)) for i, c in pairs]
        if any(len(row) != n or any(not -1 <= c < K for c in row) for row in slots):
            raise C.DrnError("CSC image batch: a slot row must hold one class (or -1) per image")
        if len(set(pairs)) != len(pairs) or any(not (0 <= i < n and 0 <= c < K) for i, c in pairs):
            raise C.DrnError("CSC image batch: the (image, class) pairs must be distinct and in range")
        self.n_img, self.K, self.sizes, self.slots, self.pairs = n, int(K), sizes, slots, pairs
        self.Hmax, self.Wmax = max(h for h, _ in sizes), max(w for _, w in sizes)
        self.max_px = max(h * w for h, w in sizes)
        self.map_off, off = [], 0
        for h, w in sizes:
            self.map_off.append(off)
            off += K * h * w
        self.map_floats = off
        self.tab_off, off = [], 0
        for i, _ in pairs:
            self.tab_off.append(off)
            off += sizes[i][0] * sizes[i][1]
        self.table_floats = off
        words = [v for hw in sizes for v in hw] + self.map_off + [c for row in slots for c in row]
        words += [v for p in pairs for v in p] + self.tab_off
        dev = torch.tensor(words, dtype=torch.int64).to(device, non_blocking=True)  # the step's one schedule upload
        S, P = len(slots), len(pairs)
        o = 0
        self.d_hw = dev[o: o + 2 * n]; o += 2 * n
        self.d_map_off = dev[o: o + n]; o += n
        self.d_slot_rows = dev[o: o + S * n]  # all slot rows [S, n] at once (a view: what drn_csc_stats reads)
        self.d_slots = [dev[o + j * n: o + (j + 1) * n] for j in range(S)]; o += S * n
        self.d_pairs = dev[o: o + 2 * P]; o += 2 * P
        self.d_tab_off = dev[o: o + P]
        self.words = dev

    def new_maps(self, device):
        """zero maps of every image -> (flat buffer, list of [K, H_i, W_i] views)"""
        flat = torch.zeros((self.map_floats,), dtype=torch.float32, device=device)
        return flat, self.map_views(flat)

    def map_views(self, flat):
        K = self.K
        return [flat[o: o + K * h * w].view(K, h, w) for o, (h, w) in zip(self.map_off, self.sizes)]

    def table_views(self, tables):
        return [tables[o: o + self.sizes[i][0] * self.sizes[i][1]].view(self.sizes[i])
                for o, (i, _) in zip(self.tab_off, self.pairs)]


def csc_seed_batch(logits, c_cls, c_det, K, scores, rowsm, img_off, n_img, slot_cls, dlogits):
    """drn_csc_seed_batch: per image d (sum of the image's rows of s[r, slot_cls[i]]) / d logits into its rows of dlogits
    (zeros where slot_cls[i] = -1).  img_off int32 [n_img + 1] and slot_cls int64 [n_img] on the device."""
    csc_batch_limits(n_img, K)
    assert img_off.dtype == torch.int32 and img_off.numel() == n_img + 1 and img_off.is_contiguous()
    assert slot_cls.dtype == torch.int64 and slot_cls.numel() == n_img and slot_cls.is_contiguous()
    assert scores.is_contiguous() and rowsm.is_contiguous()
    C.call("drn_csc_seed_batch", C.ptr(logits), _2d(logits), c_cls, c_det, K, C.ptr(scores), C.ptr(rowsm), C.ptr(img_off),
           int(n_img), scores.shape[0], C.ptr(slot_cls), C.ptr(dlogits), _2d(dlogits), C.stream())
    return dlogits


def csc_cpg_batch(dimg_nhwc, n_colours, plan, slot, maps):
    """drn_csc_cpg_batch: the padded gradient [n, Hmax, Wmax, Cpad] -> for every image with a class in slot `slot` of `plan`
    the normalised map of its own crop, into `maps` (plan.new_maps)"""
    csc_batch_limits(plan.n_img, plan.K)
    n, H, W, cp = dimg_nhwc.shape
    if n != plan.n_img or H < plan.Hmax or W < plan.Wmax:
        raise C.DrnError("CSC image batch: the gradient %s does not hold %d images of up to %d x %d" % (
            tuple(dimg_nhwc.shape), plan.n_img, plan.Hmax, plan.Wmax))
    assert dimg_nhwc.is_contiguous() and maps.is_contiguous() and maps.numel() == plan.map_floats
    scratch = torch.empty((n,), dtype=torch.int32, device=dimg_nhwc.device)
    C.call("drn_csc_cpg_batch", C.ptr(dimg_nhwc), C.dt(dimg_nhwc.dtype), cp, n_colours, n, H, W, C.ptr(plan.d_hw),
           C.ptr(plan.d_slots[slot]), plan.K, C.ptr(plan.d_map_off), C.ptr(maps), C.ptr(scratch), C.stream())
    return maps


def csc_weights_batch(maps, plan, fg_threshold, rois5, img_off, scores, area_sqrt, context_scale, W_out, tables=None):
    """drn_csc_weights_batch: every (image, class) pair of `plan` -> its column of its image's rows of W_out [M, K].
    Returns the tables scratch (plan.table_views: the summed-area table of every pair)."""
    csc_batch_limits(plan.n_img, plan.K, plan.sizes)
    M, K = scores.shape
    assert K == plan.K and W_out.shape == (M, K) and maps.numel() == plan.map_floats
    assert maps.is_contiguous() and rois5.is_contiguous() and scores.is_contiguous() and W_out.is_contiguous()
    assert img_off.dtype == torch.int32 and img_off.numel() == plan.n_img + 1
    if tables is None:
        tables = torch.empty((max(1, plan.table_floats),), dtype=torch.float32, device=scores.device)
    assert tables.numel() >= plan.table_floats
    if plan.pairs:
        C.call("drn_csc_weights_batch", C.ptr(maps), C.ptr(plan.d_map_off), C.ptr(plan.d_hw), plan.n_img, plan.Hmax, plan.Wmax,
               plan.max_px, C.ptr(plan.d_pairs), C.ptr(plan.d_tab_off), len(plan.pairs), float(fg_threshold), C.ptr(rois5),
               C.ptr(img_off), M, C.ptr(scores), K, int(area_sqrt), float(context_scale), C.ptr(tables), C.ptr(W_out),
               C.stream())
    return tables


def csc_loss_batch(logits, c_cls, c_det, K, scores, rowsm, W, onehot, img_off, n_img, mean_loss, dlogits=None):
    """drn_csc_loss_batch -> (loss_img [n_img, 2], loss [2]): per image the single-image losses, their mean over the images
    (fp64 sum in ascending order, rounded once), and the 1 / n_img-scaled dlogits rows.  W None = ones."""
    csc_batch_limits(n_img, K)
    M = scores.shape[0]
    assert onehot.shape == (n_img, K) and onehot.dtype == torch.float32 and onehot.is_contiguous()
    assert img_off.dtype == torch.int32 and img_off.numel() == n_img + 1
    assert scores.is_contiguous() and rowsm.is_contiguous() and (W is None or W.is_contiguous())
    loss_img = torch.empty((n_img, 2), dtype=torch.float32, device=scores.device)
    loss = torch.empty((2,), dtype=torch.float32, device=scores.device)
    C.call("drn_csc_loss_batch", C.ptr(logits), _2d(logits), c_cls, c_det, K, C.ptr(scores), C.ptr(rowsm), C.ptr(W),
           C.ptr(onehot), C.ptr(img_off), int(n_img), M, int(mean_loss), C.ptr(loss_img), C.ptr(loss), C.ptr(dlogits),
           _2d(dlogits) if dlogits is not None else 0, C.stream())
    return loss_img, loss


# the table of drn_csc_stats (include/drn_wsod.h, "CSC weight statistics"): 8-byte words, two int64 head words, then [field][K]
CSC_STATS_HEAD = ("steps", "num_img")
CSC_STATS_INT = ("ori_label", "ori_num_roi", "csc_label", "csc_num_roi", "csc_roi_pos", "csc_roi_neg", "csc_roi_zero")
CSC_STATS_FP = ("ori_pred", "csc_pred", "csc_pred_pos", "csc_pred_neg")


def csc_stats_words(K):
    return len(CSC_STATS_HEAD) + (len(CSC_STATS_INT) + len(CSC_STATS_FP)) * int(K)


def csc_stats_scratch_words(n_img, K):
    return int(n_img) * (1 + 6 * int(K))


def csc_stats(scores, W, img_off, n_img, onehot, slots, table, scratch=None):
    """drn_csc_stats: add one training forward's weight statistics to `table` (int64 [csc_stats_words(K)], zeroed by its owner).
    scores / W [M, K] fp32, img_off int32 [n_img + 1], onehot fp32 [n_img, K]; slots: DEVICE int64 [n_slots, n_img] - the class
    image i builds a map for in slot j, -1 = none (CscBatchPlan.d_slot_rows; a single image: its active classes) - or None."""
    M, K = scores.shape
    csc_batch_limits(n_img, K)
    n_slots = 0 if slots is None else slots.numel() // int(n_img)
    if W is None or W.shape != scores.shape or n_slots > K:
        raise C.DrnError("csc_stats: W %s for scores %s, %d slot rows" % (None if W is None else tuple(W.shape),
                                                                         tuple(scores.shape), n_slots))
    assert scores.dtype == torch.float32 and W.dtype == torch.float32 and scores.is_contiguous() and W.is_contiguous()
    assert onehot.numel() == n_img * K and onehot.dtype == torch.float32 and onehot.is_contiguous()
    assert img_off.dtype == torch.int32 and img_off.numel() == n_img + 1 and img_off.is_contiguous()
    assert table.dtype == torch.int64 and table.numel() == csc_stats_words(K) and table.is_contiguous()
    if n_slots:
        assert slots.dtype == torch.int64 and slots.numel() == n_slots * n_img and slots.is_contiguous()
    if scratch is None:
        scratch = torch.empty((csc_stats_scratch_words(n_img, K),), dtype=torch.int64, device=scores.device)
    assert scratch.dtype == torch.int64 and scratch.numel() >= csc_stats_scratch_words(n_img, K)
    C.call("drn_csc_stats", C.ptr(scores), C.ptr(W), K, C.ptr(img_off), int(n_img), M, C.ptr(onehot),
           C.ptr(slots) if n_slots else None, n_slots, C.ptr(scratch), C.ptr(table), C.stream())
    return table


def oicr_targets(prev_scores, prev_boxes, props, img_off, n_img, gt_classes, gt_count, img_scores, K,
                 thresholds=(0.5,), labels=(0, 1), zero_delta_decode=False, out=None):
    """`out`: the six output tensors, given by the caller (contiguous, at least the shapes below); allocated if None."""
    M = props.shape[0]
    dev = props.device
    gmax = gt_classes.shape[1]
    shapes = dict(labels=((M,), torch.int32), weights=((M,), torch.float32), matched=((M,), torch.int32),
                  gt_boxes=((M, 4), torch.float32), pgt_idx=((n_img, gmax), torch.int32),
                  pgt_boxes=((n_img, gmax, 4), torch.float32))
    if out is None:
        out = {k: torch.empty(s, dtype=dt, device=dev) for k, (s, dt) in shapes.items()}
    for k, (s, dt) in shapes.items():
        t = out[k]
        assert t.dtype == dt and t.is_contiguous() and t.dim() == len(s) and t.shape[0] >= s[0] and t.shape[1:] == s[1:], k
    th, lb = C.host_floats(thresholds), C.host_ints(labels)
    C.call("drn_oicr_targets", C.ptr(prev_scores), _2d(prev_scores), C.ptr(prev_boxes), prev_boxes.shape[1],
           int(zero_delta_decode), C.ptr(props),
           C.ptr(img_off), n_img, C.ptr(gt_classes), C.ptr(gt_count), gmax, C.ptr(img_scores), K,
           ctypes.cast(th, ctypes.c_void_p), ctypes.cast(lb, ctypes.c_void_p), len(thresholds), C.ptr(out["labels"]),
           C.ptr(out["weights"]), C.ptr(out["matched"]), C.ptr(out["gt_boxes"]), C.ptr(out["pgt_idx"]),
           C.ptr(out["pgt_boxes"]), C.stream())
    return out


def oicr_refine_chain(logits, col0s, K, scores0, props, img_off, n_img, gt_classes, gt_count, img_scores,
                      thresholds=(0.5,), labels=(0, 1), dlogits=None, loss_scale=1.0):
    """All (non-regressing) refinement branches at once; returns per-head (targets dict, probs, loss) views."""
    M, dev, nh = props.shape[0], props.device, len(col0s)
    gmax = gt_classes.shape[1]
    nb = (M + 15) // 16
    e = lambda shape, dt: torch.empty(shape, dtype=dt, device=dev)
    probs = e((nh, M, K + 1), torch.float32)
    out = dict(labels=e((nh, M), torch.int32), weights=e((nh, M), torch.float32), matched=e((nh, M), torch.int32),
               gt_boxes=e((nh, M, 4), torch.float32), pgt_idx=e((nh, n_img, gmax), torch.int32),
               pgt_boxes=e((nh, n_img, gmax, 4), torch.float32))
    losses = e((nh,), torch.float32)
    scratch = e((nh * 2 * nb,), torch.float32)
    th, lb, c0 = C.host_floats(thresholds), C.host_ints(labels), C.host_ints(col0s)
    vp = lambda a: ctypes.cast(a, ctypes.c_void_p)
    C.call("drn_oicr_refine_chain", C.ptr(logits), _2d(logits), vp(c0), nh, K, C.ptr(scores0), _2d(scores0),
           C.ptr(props), C.ptr(img_off), n_img, C.ptr(gt_classes), C.ptr(gt_count), gmax, C.ptr(img_scores),
           vp(th), vp(lb), len(thresholds),
           C.ptr(probs), C.ptr(out["labels"]), C.ptr(out["weights"]), C.ptr(out["matched"]), C.ptr(out["gt_boxes"]),
           C.ptr(out["pgt_idx"]), C.ptr(out["pgt_boxes"]),
           C.ptr(dlogits), _2d(dlogits) if dlogits is not None else 0, C.ptr(losses), C.ptr(scratch), M,
           float(loss_scale), C.stream())
    return [({k: v[i] for k, v in out.items()}, probs[i], losses[i: i + 1]) for i in range(nh)]


def mil_oicr_losses(partials, bias, logits, c_cls, c_det, K, img_off, n_img, gt_onehot, col0s, props, gt_classes,
                    gt_count, thresholds=(0.5,), labels=(0, 1), dlogits=None, mean_loss=True, loss_scale=1.0,
                    max_rows=None, seed_inc=0, seed_dev=None):
    """drn_mil_oicr_losses: predictor split-K reduce + bias -> `logits` (written), WSDDN forward/backward and the whole
    non-regressing refinement cascade in six launches.  Returns (scores, img_scores, loss_part, chain) with `chain` as
    oicr_refine_chain returns it."""
    M, dev, nh = props.shape[0], props.device, len(col0s)
    max_rows = max_rows or M
    gmax = gt_classes.shape[1]
    nb = (M + 15) // 16
    e = lambda shape, dt: torch.empty(shape, dtype=dt, device=dev)
    scores, rowsm = e((M, K), torch.float32), e((M, K), torch.float32)
    img_scores, loss_part = e((n_img, K), torch.float32), e((n_img,), torch.float32)
    ws_scratch = e((n_img * ((max_rows + 31) // 32) * 384,), torch.float32)
    probs = e((nh, M, K + 1), torch.float32)
    out = dict(labels=e((nh, M), torch.int32), weights=e((nh, M), torch.float32), matched=e((nh, M), torch.int32),
               gt_boxes=e((nh, M, 4), torch.float32), pgt_idx=e((nh, n_img, gmax), torch.int32),
               pgt_boxes=e((nh, n_img, gmax, 4), torch.float32))
    losses = e((nh,), torch.float32)
    ce_scratch = e((nh * 2 * nb,), torch.float32)
    th, lb, c0 = C.host_floats(thresholds), C.host_ints(labels), C.host_ints(col0s)
    vp = lambda a: ctypes.cast(a, ctypes.c_void_p)
    splits = partials.shape[0] if partials.dim() == 3 else 1
    sstride = partials.stride(0) if partials.dim() == 3 else 0
    C.call("drn_mil_oicr_losses", C.ptr(partials), splits, sstride, partials.stride(-2), C.ptr(bias), int(seed_inc),
           C.ptr(seed_dev), C.ptr(logits), _2d(logits), c_cls, c_det, K, C.ptr(img_off), n_img, C.ptr(gt_onehot),
           C.ptr(scores), C.ptr(rowsm), C.ptr(img_scores), C.ptr(loss_part), C.ptr(ws_scratch), int(max_rows),
           int(mean_loss), vp(c0), nh, C.ptr(props), C.ptr(gt_classes), C.ptr(gt_count), gmax, vp(th), vp(lb),
           len(thresholds), C.ptr(probs), C.ptr(out["labels"]), C.ptr(out["weights"]), C.ptr(out["matched"]),
           C.ptr(out["gt_boxes"]), C.ptr(out["pgt_idx"]), C.ptr(out["pgt_boxes"]), C.ptr(losses), C.ptr(ce_scratch),
           C.ptr(dlogits), _2d(dlogits) if dlogits is not None else 0, M, float(loss_scale), C.stream())
    chain = [({k: v[i] for k, v in out.items()}, probs[i], losses[i: i + 1]) for i in range(nh)]
    return scores, img_scores, loss_part, chain


def softmax_ce(logits, col0, ncol, labels=None, weights=None, dlogits=None, loss_scale=1.0):
    M = logits.shape[0]
    probs = torch.empty((M, ncol), dtype=torch.float32, device=logits.device)
    loss = torch.empty((1,), dtype=torch.float32, device=logits.device) if labels is not None else None
    scratch = torch.empty((2 * ((M + 15) // 16),), dtype=torch.float32, device=logits.device) if labels is not None else None
    C.call("drn_softmax_ce", C.ptr(logits), _2d(logits), col0, ncol, C.ptr(labels), C.ptr(weights), C.ptr(probs),
           C.ptr(dlogits), _2d(dlogits) if dlogits is not None else 0, C.ptr(loss), C.ptr(scratch), M, float(loss_scale),
           C.stream())
    return probs, loss


def box_reg_loss(logits, col0, K, labels, props, gt_boxes, weights=(10.0, 10.0, 5.0, 5.0), dlogits=None, loss_scale=1.0):
    M = logits.shape[0]
    loss = torch.zeros((1,), dtype=torch.float32, device=logits.device)
    scratch = torch.empty(((M + 255) // 256,), dtype=torch.float32, device=logits.device)
    w = C.host_floats(weights)
    C.call("drn_box_reg_loss", C.ptr(logits), _2d(logits), col0, K, C.ptr(labels), C.ptr(props), C.ptr(gt_boxes),
           ctypes.cast(w, ctypes.c_void_p), C.ptr(dlogits), _2d(dlogits) if dlogits is not None else 0, C.ptr(loss),
           C.ptr(scratch), M, float(loss_scale), C.stream())
    return loss


_COL0_DEV = {}
COL0_CACHE = True  # tools: False = the column table is uploaded per call (a host sync per inference pass)


def mean_softmax(logits, col0s, ncol, bg_first=False):
    M = logits.shape[0]
    probs = torch.empty((M, ncol), dtype=torch.float32, device=logits.device)
    # the column table lives on the device once per (columns, device): built per call it was a pageable H2D copy, which waits for
    # the stream's queued work - every inference pass ended in a host sync (1.3 ms of a TTA pass, profiles/r5_53_tta_host_profile.txt)
    key = (tuple(int(c) for c in col0s), str(logits.device))
    cd = _COL0_DEV.get(key) if COL0_CACHE else None
    if cd is None:
        cd = _COL0_DEV[key] = torch.tensor(list(key[0]), dtype=torch.int32, device=logits.device)
    C.call("drn_mean_softmax", C.ptr(logits), _2d(logits), C.ptr(cd), len(col0s), ncol, C.ptr(probs), M, int(bg_first),
           C.stream())
    return probs


def apply_deltas(deltas, boxes, K, weights=(10.0, 10.0, 5.0, 5.0), col0=0):
    """deltas: [M, ld] fp32 (class-specific deltas start at column col0) or None (zeros) -> [M, 4K]."""
    M = boxes.shape[0]
    out = torch.empty((M, 4 * K), dtype=torch.float32, device=boxes.device)
    w = C.host_floats(weights)
    dp = None if deltas is None else deltas.data_ptr() + 4 * col0
    C.call("drn_apply_deltas", dp, _2d(deltas) if deltas is not None else 0, C.ptr(boxes), C.ptr(out), M, K,
           ctypes.cast(w, ctypes.c_void_p), float(SCALE_CLAMP), C.stream())
    return out


BOXREG_MAX_HEADS, BOXREG_MAX_IMAGES = 8, 16  # include/drn_wsod.h


def apply_deltas_mean(logits, col0s, n_total, boxes, K, weights=(10.0, 10.0, 5.0, 5.0)):
    """drn_apply_deltas_mean: boxes decoded from the mean of n_total branches' deltas, of which the branches at columns `col0s`
    (ascending; may be empty) regress and the others contribute zeros (PCLROIHeads' inference, predict_boxes_K) -> [M, 4K]."""
    M = boxes.shape[0]
    out = torch.empty((M, 4 * K), dtype=torch.float32, device=boxes.device)
    w, cz = C.host_floats(weights), C.host_ints(col0s)
    C.call("drn_apply_deltas_mean", C.ptr(logits) if len(col0s) else None, _2d(logits) if len(col0s) else 0,
           ctypes.cast(cz, ctypes.c_void_p), len(col0s), int(n_total), C.ptr(boxes), C.ptr(out), M, K,
           ctypes.cast(w, ctypes.c_void_p), float(SCALE_CLAMP), C.stream())
    return out


def annot_box_reg(logits, col0s, K, props, img_off, n_img, gt_boxes, gt_classes, gt_count, thresholds=(0.5,), labels=(0, 1),
                  weights=(10.0, 10.0, 5.0, 5.0), dlogits=None, loss_scale=1.0, max_rows=None, want_labels=False):
    """drn_annot_box_reg: loss_box_reg of the regressing PCL branches at delta columns `col0s` against the ANNOTATED boxes (the
    label_proposals() labelling, get_deltas targets, L1 / M_i, mean over the images), fused with its dlogits - one launch pair for
    all branches and images.  -> loss fp32 [len(col0s)], or (loss, labels, matched) with want_labels.  No synchronisation;
    capturable."""
    M, dev = props.shape[0], props.device
    max_gt, nthr, nh = gt_classes.shape[1], len(thresholds), len(col0s)
    if (max_gt > LABEL_MAX_GT or not 1 <= nthr <= 3 or len(labels) != nthr + 1 or not 1 <= nh <= BOXREG_MAX_HEADS or
            n_img > BOXREG_MAX_IMAGES):
        raise C.DrnError("annot_box_reg(): max_gt %d, %d thresholds, %d labels, %d branches, %d images (at most %d boxes per image, "
                         "1 .. 3 thresholds and one label more, 1 .. %d branches, %d images are built)"
                         % (max_gt, nthr, len(labels), nh, n_img, LABEL_MAX_GT, BOXREG_MAX_HEADS, BOXREG_MAX_IMAGES))
    assert logits.dtype == torch.float32 and logits.dim() == 2 and logits.stride(1) == 1 and logits.shape[0] >= M
    assert props.dtype == torch.float32 and props.dim() == 2 and props.shape[1] == 4 and props.is_contiguous()
    assert img_off.dtype == torch.int32 and img_off.numel() == n_img + 1 and img_off.is_contiguous()
    assert gt_boxes.dtype == torch.float32 and gt_boxes.shape == (n_img, max_gt, 4) and gt_boxes.is_contiguous()
    assert gt_classes.dtype == torch.int32 and gt_classes.shape == (n_img, max_gt) and gt_classes.is_contiguous()
    assert gt_count.dtype == torch.int32 and gt_count.numel() == n_img and gt_count.is_contiguous()
    if dlogits is not None:
        assert dlogits.dtype == torch.float32 and dlogits.dim() == 2 and dlogits.stride(1) == 1 and dlogits.shape[0] >= M
    max_rows = int(max_rows or M)
    loss = torch.zeros((nh,), dtype=torch.float32, device=dev)
    scratch = torch.empty((max(1, nh * n_img * ((max_rows + 255) // 256)),), dtype=torch.float32, device=dev)
    lab = torch.empty((M,), dtype=torch.int32, device=dev) if want_labels else None
    mat = torch.empty((M,), dtype=torch.int32, device=dev) if want_labels else None
    th, lb, w, cz = C.host_floats(thresholds), C.host_ints(labels), C.host_floats(weights), C.host_ints(col0s)
    C.call("drn_annot_box_reg", C.ptr(logits), _2d(logits), ctypes.cast(cz, ctypes.c_void_p), nh, int(K), C.ptr(props),
           C.ptr(img_off), int(n_img), M, max_rows, C.ptr(gt_boxes), C.ptr(gt_classes), C.ptr(gt_count), max_gt,
           ctypes.cast(th, ctypes.c_void_p), ctypes.cast(lb, ctypes.c_void_p), nthr, ctypes.cast(w, ctypes.c_void_p),
           C.ptr(dlogits), _2d(dlogits) if dlogits is not None else 0, float(loss_scale), C.ptr(loss), C.ptr(lab), C.ptr(mat),
           C.ptr(scratch), C.stream())
    return (loss, lab, mat) if want_labels else loss


def sum_small(x, scale=1.0):
    out = torch.empty((1,), dtype=torch.float32, device=x.device)
    C.call("drn_sum_small", C.ptr(x), x.numel(), float(scale), C.ptr(out), C.stream())
    return out


GUARD_RAISE, GUARD_SKIP = 1, 2  # mode of drn_loss_guard
GUARD_MAX_LOSSES = 16


def loss_guard_state(device):
    """int32[4] state of loss_guard() as the first call expects it: {skip flag 0, calls 0, first bad call -1, bad calls 0}"""
    return torch.tensor([0, 0, -1, 0], dtype=torch.int32, device=device)


def _guard_ptr(state):
    assert state.dtype == torch.int32 and state.numel() >= 1 and state.is_contiguous()
    return C.ptr(state)


def loss_guard(losses, mode, window_first, state):
    """drn_loss_guard: one wave sums the step's fp32 loss scalars (device tensors of one element, at most 16) in list order and
    folds isfinite(sum) into `state` (loss_guard_state()): [0] the skip flag the guarded updates read, [1] calls, [2] first bad
    call or -1, [3] bad calls.  mode GUARD_RAISE: sticky flag; GUARD_SKIP: flag = bad_now or (flag and not window_first).  No
    synchronisation; capturable."""
    n = len(losses)
    if not 1 <= n <= GUARD_MAX_LOSSES:
        raise C.DrnError("loss_guard(): %d loss scalars (1 .. %d are built)" % (n, GUARD_MAX_LOSSES))
    for t in losses:
        assert t.dtype == torch.float32 and t.numel() == 1 and t.is_cuda
    assert state.dtype == torch.int32 and state.numel() == 4 and state.is_contiguous()
    ptrs = (ctypes.c_void_p * n)(*[t.data_ptr() for t in losses])
    C.call("drn_loss_guard", ctypes.cast(ptrs, ctypes.c_void_p), n, int(mode), int(bool(window_first)), C.ptr(state),
           C.stream())


# include/drn_wsod.h: DRN_METRICS_*
METRICS_MAX_HEADS, METRICS_MAX_LOSSES, METRICS_COUNTERS, METRICS_COUNT_STRIDE = 8, 16, 6, 8
METRICS_ROWS_PER_BLOCK, METRICS_RECORD_WORDS = 64, 72


def head_metrics_rows(K):
    """(rows one wave of drn_head_metrics holds at a time, rows of one workgroup) for K foreground classes"""
    lanes = 2
    while lanes < 64 and lanes < (K + 7) // 4:
        lanes *= 2
    return 64 // lanes, METRICS_ROWS_PER_BLOCK


def metrics_ring(slots, device):
    """Device side of the per-step metrics: ONE int32 allocation [4 + slots * METRICS_RECORD_WORDS] (so a drain is one copy), its
    views `state` (int32[4], [0] = records written) and `ring` ([slots, METRICS_RECORD_WORDS]), and the zeroed counts scratch
    of head_metrics() (int32[METRICS_MAX_HEADS, METRICS_COUNT_STRIDE])."""
    slots = int(slots)
    if slots < 1:
        raise C.DrnError("metrics_ring(): %d slots" % slots)
    buf = torch.zeros((4 + slots * METRICS_RECORD_WORDS,), dtype=torch.int32, device=device)
    return dict(buf=buf, state=buf[:4], ring=buf[4:].view(slots, METRICS_RECORD_WORDS),
                counts=torch.zeros((METRICS_MAX_HEADS, METRICS_COUNT_STRIDE), dtype=torch.int32, device=device))


def head_metrics(logits, col0s, K, labels, M, counts):
    """drn_head_metrics: per refinement branch k, the six label counters of rows 0 .. M-1 - n_ig, n_bg, n_fg, n_acc, n_fg_acc,
    n_fneg with p = first arg-max of logits[r, col0s[k] : col0s[k] + K + 1] and g = labels[k][r] - ADDED into counts[k, 0:6]
    (zero on entry; metrics_record() clears it again).  labels: an int32 [nh, M] tensor or a list of nh int32 [M] tensors."""
    nh = len(col0s)
    if nh > METRICS_MAX_HEADS or K + 1 > 1024:
        raise C.DrnError("head_metrics(): %d branches of %d columns (at most %d of at most 1024 are built)"
                         % (nh, K + 1, METRICS_MAX_HEADS))
    assert logits.dtype == torch.float32 and logits.dim() == 2 and logits.stride(1) == 1 and logits.shape[0] >= M
    assert counts.dtype == torch.int32 and counts.is_contiguous() and counts.numel() == METRICS_MAX_HEADS * METRICS_COUNT_STRIDE
    rows = [labels[k] for k in range(nh)]
    assert len(labels) == nh
    for t in rows:
        assert t.dtype == torch.int32 and t.is_cuda and t.is_contiguous() and t.numel() >= M
    ptrs = (ctypes.c_void_p * max(nh, 1))(*[t.data_ptr() for t in rows])
    c0 = C.host_ints(list(col0s) or [0])
    C.call("drn_head_metrics", C.ptr(logits), _2d(logits), ctypes.cast(c0, ctypes.c_void_p), nh, int(K),
           ctypes.cast(ptrs, ctypes.c_void_p), int(M), C.ptr(counts), C.stream())


def metrics_record(losses, counts, nh, M, ring, state, annot=False):
    """drn_metrics_record: one wave writes the step's record - index, n, nh, M, the loss bit patterns, counts[:nh, 0:6], index again -
    into slot state[0] % slots of `ring`, advances state[0] and stores zeros back into `counts`.  No synchronisation; capturable.
    annot (drn_metrics_record_annot): counts[METRICS_ANNOT_ROW] - what label_proposals() and mil_metrics() added - is published too,
    in the last head slot, word 68 and the flag word 70; nh may then be at most 7."""
    n = len(losses)
    if not 1 <= n <= METRICS_MAX_LOSSES or nh > (METRICS_ANNOT_ROW if annot else METRICS_MAX_HEADS):
        raise C.DrnError("metrics_record(): %d loss scalars, %d branches (1 .. %d and 0 .. %d are built)"
                         % (n, nh, METRICS_MAX_LOSSES, METRICS_ANNOT_ROW if annot else METRICS_MAX_HEADS))
    for t in losses:
        assert t.dtype == torch.float32 and t.numel() == 1 and t.is_cuda
    assert ring.dtype == torch.int32 and ring.dim() == 2 and ring.shape[1] == METRICS_RECORD_WORDS and ring.is_contiguous()
    assert state.dtype == torch.int32 and state.numel() == 4 and state.is_contiguous()
    assert counts.dtype == torch.int32 and counts.is_contiguous() and counts.numel() == METRICS_MAX_HEADS * METRICS_COUNT_STRIDE
    ptrs = (ctypes.c_void_p * n)(*[t.data_ptr() for t in losses])
    if annot:
        C.call("drn_metrics_record_annot", ctypes.cast(ptrs, ctypes.c_void_p), n, C.ptr(counts), int(nh), int(M), 1, C.ptr(ring),
               ring.shape[0], C.ptr(state), C.stream())
        return
    C.call("drn_metrics_record", ctypes.cast(ptrs, ctypes.c_void_p), n, C.ptr(counts), int(nh), int(M), C.ptr(ring),
           ring.shape[0], C.ptr(state), C.stream())


# include/drn_wsod.h: the annotated-box block
LABEL_MAX_GT, METRICS_ANNOT_ROW, METRICS_ANNOT_WORD_FG, METRICS_ANNOT_WORD_FLAG, METRICS_ANNOT_FLAG = 256, 7, 68, 70, 1


def label_proposals(props, img_off, n_img, gt_boxes, gt_classes, gt_count, K, thresholds=(0.5,), labels=(0, 1), counts=None,
                    max_rows=None, out=None):
    """drn_label_proposals: every proposal row against the ANNOTATED boxes of its image (pairwise_iou + Matcher without low-quality
    matches + the matched box's class; roi_heads.py:256-353).  props fp32 [M, 4], img_off int32 [n_img + 1], gt_boxes fp32
    [n_img, max_gt, 4], gt_classes int32 [n_img, max_gt], gt_count int32 [n_img].  -> dict(labels int32 [M]: class, K background,
    -1 ignore; matched int32 [M]: the best box, lowest index on equal IoU; counts: n_ig, n_bg, n_fg ADDED into counts[0:3]).
    counts: an int32 block of >= 3 words (a zeroed one of METRICS_COUNT_STRIDE is made when None); out: (labels, matched) to write
    into.  No synchronisation; capturable."""
    M, dev = props.shape[0], props.device
    max_gt = gt_classes.shape[1]
    nthr = len(thresholds)
    if max_gt > LABEL_MAX_GT or not 1 <= nthr <= 3 or len(labels) != nthr + 1:
        raise C.DrnError("label_proposals(): max_gt %d, %d thresholds, %d labels (at most %d boxes per image, 1 .. 3 thresholds "
                         "and one label more are built)" % (max_gt, nthr, len(labels), LABEL_MAX_GT))
    assert props.dtype == torch.float32 and props.dim() == 2 and props.shape[1] == 4 and props.is_contiguous()
    assert img_off.dtype == torch.int32 and img_off.numel() == n_img + 1 and img_off.is_contiguous()
    assert gt_boxes.dtype == torch.float32 and gt_boxes.shape == (n_img, max_gt, 4) and gt_boxes.is_contiguous()
    assert gt_classes.dtype == torch.int32 and gt_classes.shape == (n_img, max_gt) and gt_classes.is_contiguous()
    assert gt_count.dtype == torch.int32 and gt_count.numel() == n_img and gt_count.is_contiguous()
    if counts is None:
        counts = torch.zeros((METRICS_COUNT_STRIDE,), dtype=torch.int32, device=dev)
    assert counts.dtype == torch.int32 and counts.is_contiguous() and counts.numel() >= 3
    lab, mat = out if out is not None else (torch.empty((M,), dtype=torch.int32, device=dev),
                                            torch.empty((M,), dtype=torch.int32, device=dev))
    for t in (lab, mat):
        assert t.dtype == torch.int32 and t.is_contiguous() and t.numel() >= M
    th, lb = C.host_floats(thresholds), C.host_ints(labels)
    C.call("drn_label_proposals", C.ptr(props), C.ptr(img_off), int(n_img), M, int(max_rows or M), C.ptr(gt_boxes),
           C.ptr(gt_classes), C.ptr(gt_count), max_gt, ctypes.cast(th, ctypes.c_void_p), ctypes.cast(lb, ctypes.c_void_p), nthr,
           int(K), C.ptr(lab), C.ptr(mat), C.ptr(counts), C.stream())
    return dict(labels=lab, matched=mat, counts=counts)


def mil_metrics(scores, labels, M, counts, ncol=None, bg_ind=None):
    """drn_mil_metrics: WSDDNOutputs._log_accuracy (fast_rcnn.py:213-235) of the MIL scores [>= M, ncol] against label_proposals()'
    labels, with that code's background index ncol - 1: n_acc, n_fg_acc, n_fneg and the foreground count #{0 <= g < ncol - 1} ADDED
    into counts[3:7].  First arg-max, like head_metrics().  No synchronisation; capturable."""
    ncol = scores.shape[1] if ncol is None else int(ncol)
    bg_ind = ncol - 1 if bg_ind is None else int(bg_ind)
    if ncol > 1024 or bg_ind != ncol - 1:
        raise C.DrnError("mil_metrics(): %d columns, background index %d (at most 1024 columns, background = the last, are built)"
                         % (ncol, bg_ind))
    assert scores.dtype == torch.float32 and scores.dim() == 2 and scores.stride(1) == 1 and scores.shape[0] >= M
    assert scores.shape[1] >= ncol >= 1
    assert labels.dtype == torch.int32 and labels.is_contiguous() and labels.numel() >= M
    assert counts.dtype == torch.int32 and counts.is_contiguous() and counts.numel() >= 7
    C.call("drn_mil_metrics", C.ptr(scores), _2d(scores), ncol, bg_ind, C.ptr(labels), int(M), C.ptr(counts), C.stream())


CLIP_NONE, CLIP_VALUE, CLIP_NORM = 0, 1, 2  # clip_mode of drn_sgd_step_clip / drn_sgd_step_block_clip
_NORM_TYPES = {1.0: 1, 2.0: 2, float("inf"): 0}  # NORM_TYPE -> norm_type of drn_grad_norms


def norm_type_code(norm_type):
    """SOLVER.CLIP_GRADIENTS.NORM_TYPE -> drn_grad_norms' code; 1, 2 and inf are built."""
    code = _NORM_TYPES.get(float(norm_type))
    if code is None:
        raise C.DrnError("SOLVER.CLIP_GRADIENTS.NORM_TYPE %r is not built: 1, 2 and inf are" % (norm_type,))
    return code


def grad_norms_ws_bytes(nseg):
    """bytes of the workspace drn_grad_norms needs for nseg segments (host-only)"""
    return C.lib().drn_grad_norms_ws_bytes(int(nseg))


def grad_norms(grads, segs_dev, nseg, norm_type, grad_scale=1.0, grad_off=0, out=None, workspace=None):
    """Per-segment norms || grads[segment] * grad_scale ||_p (p = norm_type: 1, 2 or inf) -> fp32 [nseg] on the device; grads /
    grad_off as in sgd_step.  No atomics, fixed summation order, no host synchronisation.  out / workspace (uint8,
    grad_norms_ws_bytes(nseg)): buffers to reuse, e.g. under a captured graph."""
    code = norm_type_code(norm_type)
    if out is None:
        out = torch.empty((nseg,), dtype=torch.float32, device=grads.device)
    need = grad_norms_ws_bytes(nseg)
    if workspace is None:
        workspace = torch.empty((need,), dtype=torch.uint8, device=grads.device)
    C.call("drn_grad_norms", C.ptr(grads), C.dt(grads.dtype), int(grad_off), C.ptr(segs_dev), int(nseg), code,
           float(grad_scale), C.ptr(out), C.ptr(workspace), int(workspace.numel() * workspace.element_size()), C.stream())
    return out


def _clip_args(clip):
    mode, value, norms = clip
    mode = int(mode)
    if mode == CLIP_NORM and norms is None:
        raise C.DrnError("clip=(CLIP_NORM, value, norms) needs the device norms of grad_norms()")
    return mode, float(value), C.ptr(norms) if mode == CLIP_NORM else None


def _sgd_call(entry, common, clip, guard):
    """entry(common..., stream), entry_clip(common..., clip..., stream) or entry_guard(common..., clip..., guard, stream); a guard
    without clipping passes clip_mode CLIP_NONE"""
    if guard is not None:
        C.call(entry + "_guard", *common, *_clip_args(clip if clip is not None else (CLIP_NONE, 0.0, None)), _guard_ptr(guard),
               C.stream())
    elif clip is not None:
        C.call(entry + "_clip", *common, *_clip_args(clip), C.stream())
    else:
        C.call(entry, *common, C.stream())


_SGD_SEG = np.dtype([("off", "<i8"), ("cnt", "<i8"), ("lr", "<f4"), ("wd", "<f4")])  # struct SgdSeg (csrc/drn_common.h)


def sgd_segments(rows, out=None, device="cuda"):
    """The device segment table of sgd_step / sgd_step_block / grad_norms / gemm_tn_sgd: rows = iterable of (off, cnt, lr, wd), one
    struct SgdSeg each, as a uint8 tensor.  out: the table to overwrite IN PLACE instead (same number of rows; a captured graph
    keeps reading it) - returned; device: where a new table goes."""
    rows = list(rows)
    arr = np.zeros(len(rows), dtype=_SGD_SEG)
    for i, r in enumerate(rows):
        arr[i] = tuple(r)
    host = torch.from_numpy(arr.view(np.uint8))
    if out is None:
        return host.to(device)
    out.copy_(host)
    return out


def sgd_step(weights, momentum_buf, grads, segs_dev, nseg, momentum, first_step, grad_scale=1.0, shadow=None,
             grad_off=0, clip=None, guard=None):
    """grads: the fp32 gradient arena, or (grad_off > 0) a bucket buffer - fp32 or bf16 - whose element 0 is arena
    element grad_off.  clip = (mode, value, norms): SOLVER.CLIP_GRADIENTS per segment on g * grad_scale (drn_sgd_step_clip;
    norms = grad_norms() over the same table for CLIP_NORM); None = drn_sgd_step.  guard: the int32 state of loss_guard()
    (drn_sgd_step_guard: a set flag leaves weights / momentum_buf / shadow bit-unchanged); None = the unguarded entry points."""
    if HBM_TIMING is not None:
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
    _sgd_call("drn_sgd_step", (C.ptr(weights), C.ptr(momentum_buf), C.ptr(grads), C.dt(grads.dtype), int(grad_off), C.ptr(shadow),
                               C.dt(shadow.dtype) if shadow is not None else 0, C.ptr(segs_dev), nseg, float(momentum),
                               int(first_step), float(grad_scale)), clip, guard)
    if HBM_TIMING is not None:
        e1.record()
        # bytes are the caller's to know (the segment table lives on the device): keyed by (segments, bucket offset)
        HBM_TIMING.append((e0, e1, None, ("sgd", int(nseg), int(grad_off), str(grads.dtype), shadow is not None)))


def sgd_step_block(weights, momentum_buf, grads, seg_dev, r0, rows, c0, cols, ld, momentum, first_step, grad_scale=1.0,
                   shadow=None, grad_off=0, clip=None, guard=None):
    """drn_sgd_step on rows r0 .. r0+rows, columns c0 .. c0+cols of the [., ld] tensor described by seg_dev (ONE
    {offset, count, lr, wd} entry on the device); weights / momentum_buf / shadow are the flat arenas, grads as in
    sgd_step.  clip as in sgd_step (drn_sgd_step_block_clip); its norms = ONE element, the norm of that tensor; guard as in
    sgd_step (drn_sgd_step_block_guard)."""
    if HBM_TIMING is not None:
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
    _sgd_call("drn_sgd_step_block", (C.ptr(weights), C.ptr(momentum_buf), C.ptr(grads), C.dt(grads.dtype), int(grad_off),
                                     C.ptr(shadow), C.dt(shadow.dtype) if shadow is not None else 0, C.ptr(seg_dev), int(r0),
                                     int(rows), int(c0), int(cols), int(ld), float(momentum), int(first_step),
                                     float(grad_scale)), clip, guard)
    if HBM_TIMING is not None:
        e1.record()
        HBM_TIMING.append((e0, e1, int(rows) * int(cols), ("sgd_block", int(r0), int(rows), int(c0), int(cols),
                                                            str(grads.dtype), shadow is not None)))


def detect_topk(boxes, scores, image_shape, score_thresh, nms_thresh, topk):
    """Single image: boxes [R, 4*nreg] f32, scores [R, K+1] f32 -> (boxes [n,4], scores [n], classes [n] i64,
    rows [n] i64) exactly as fast_rcnn_inference_single_image."""
    R, K = scores.shape[0], scores.shape[1] - 1
    nreg = boxes.shape[1] // 4
    dev = boxes.device
    cap = max(R * K, 1)
    nbytes = C.lib().drn_detect_workspace_bytes(cap)
    ws = torch.empty((nbytes,), dtype=torch.uint8, device=dev)
    keep = torch.empty((topk,), dtype=torch.int32, device=dev)
    nk = torch.zeros((1,), dtype=torch.int32, device=dev)
    boxes = boxes.contiguous().float()
    scores = scores.contiguous().float()
    C.call("drn_detect_topk", C.ptr(boxes), C.ptr(scores), R, K, nreg, float(image_shape[0]), float(image_shape[1]),
           float(score_thresh), float(nms_thresh), topk, C.ptr(ws), nbytes, cap, C.ptr(keep), C.ptr(nk), C.stream())
    ob = torch.empty((topk, 4), dtype=torch.float32, device=dev)
    os_ = torch.empty((topk,), dtype=torch.float32, device=dev)
    oc = torch.empty((topk,), dtype=torch.int32, device=dev)
    orow = torch.empty((topk,), dtype=torch.int32, device=dev)
    C.call("drn_detect_gather", C.ptr(ws), nbytes, cap, C.ptr(keep), C.ptr(nk), topk, C.ptr(ob), C.ptr(os_), C.ptr(oc),
           C.ptr(orow), C.stream())
    n = int(nk.item())
    return ob[:n], os_[:n], oc[:n].long(), orow[:n].long()


NMS_MAX_N = 524288  # include/drn_wsod.h DRN_NMS_MAX_N


def _device_f32(t, dev=None):
    """fp32, contiguous, on the device (a host tensor goes to `dev` or the current device) - what the entry points read"""
    if not t.is_cuda:
        t = t.to(dev if dev is not None else torch.device("cuda", torch.cuda.current_device()))
    return t.contiguous().float()


def nms_workspace_bytes(n):
    """bytes of scratch nms / batched_nms take for n boxes: DRN_NMS_WS_BYTES(n) = 104 n + 65536, linear in n"""
    return int(C.lib().drn_nms_workspace_bytes(int(n)))


def _nms(name, boxes, scores, idxs, iou_threshold, padded):
    if boxes.dim() != 2 or boxes.shape[1] != 4 or scores.dim() != 1 or scores.shape[0] != boxes.shape[0] or (
            idxs is not None and (idxs.dim() != 1 or idxs.shape[0] != boxes.shape[0])):
        raise C.DrnError("%s: boxes [n, 4], scores [n]%s expected, got %s, %s%s" % (
            name, ", idxs [n]" if idxs is not None else "", tuple(boxes.shape), tuple(scores.shape),
            ", %s" % (tuple(idxs.shape),) if idxs is not None else ""))
    n = boxes.shape[0]
    if n > NMS_MAX_N:
        raise C.DrnError("%s: %d boxes, at most %d per call are built" % (name, n, NMS_MAX_N))
    thr = float(iou_threshold)
    if thr != thr:
        raise C.DrnError("%s: the IoU threshold is NaN" % name)
    if n == 0:  # nothing to launch: the empty result is known on the host
        keep = torch.empty((0,), dtype=torch.int64, device=boxes.device)
        return (keep, torch.zeros((1,), dtype=torch.int32, device=boxes.device)) if padded else keep
    boxes = _device_f32(boxes)
    dev = boxes.device
    scores = _device_f32(scores, dev)
    nbytes = nms_workspace_bytes(n)
    ws = torch.empty((nbytes,), dtype=torch.uint8, device=dev)
    keep = torch.empty((n,), dtype=torch.int64, device=dev)
    nk = torch.empty((1,), dtype=torch.int32, device=dev)
    if idxs is None:
        C.call("drn_nms", C.ptr(boxes), C.ptr(scores), n, thr, C.ptr(ws), nbytes, C.ptr(keep), C.ptr(nk), C.stream())
    else:
        idxs = idxs.to(device=dev, dtype=torch.int32).contiguous()
        C.call("drn_batched_nms", C.ptr(boxes), C.ptr(scores), C.ptr(idxs), n, thr, C.ptr(ws), nbytes, C.ptr(keep), C.ptr(nk),
               C.stream())
    if padded:
        return keep, nk
    return keep[:int(nk.item())]


def nms(boxes, scores, iou_threshold, padded=False):
    """torchvision.ops.nms on the device (drn_nms): boxes [n, 4] XYXY, scores [n] -> the int64 indices of the kept boxes in
    descending score order (equal scores in input order; a box is dropped iff its IoU with a kept earlier one is strictly above
    the threshold; a NaN score is undefined).  padded=False returns the reference's variable-length tensor, at the price of ONE
    4-byte read of the count; padded=True returns (keep [n] int64, count [1] int32) - keep[:count] is the result, the words behind it
    are unspecified - and reads nothing back, so the call can be captured in a graph.  Input that is not fp32, not contiguous or
    not on the device is converted.  More than NMS_MAX_N boxes raise DrnError before the library is touched."""
    return _nms("nms", boxes, scores, None, iou_threshold, padded)


def batched_nms(boxes, scores, idxs, iou_threshold, padded=False):
    """detectron2.layers.batched_nms (nms.py:10-29) on the device (drn_batched_nms): boxes of different idxs never suppress each
    other - below 40000 boxes by the reference's coordinate offset idx * (boxes.max() + 1), from 40000 on per class on the raw
    boxes.  idxs: any integer dtype.  Result, padded= and limits as nms()."""
    return _nms("batched_nms", boxes, scores, idxs, iou_threshold, padded)


def detect_all(boxes, scores, image_shape, score_thresh, nms_thresh, topk=-1):
    """detect_topk without the 1024 cap (drn_detect_all): topk < 0 returns every detection that survives the NMS
    (fast_rcnn.py:65,133), topk >= 1 the first topk.  Same arguments and the same four results as detect_topk; ONE 4-byte read of the
    count.  R * K above NMS_MAX_N or topk == 0 raise DrnError before the library is touched."""
    if boxes.dim() != 2 or scores.dim() != 2 or scores.shape[0] != boxes.shape[0] or scores.shape[1] < 2:
        raise C.DrnError("detect_all: boxes [R, 4 * nreg], scores [R, K + 1] expected, got %s, %s"
                         % (tuple(boxes.shape), tuple(scores.shape)))
    R, K = scores.shape[0], scores.shape[1] - 1
    nreg = boxes.shape[1] // 4
    topk = int(topk)
    if topk == 0 or boxes.shape[1] != 4 * nreg or nreg not in (1, K):
        raise C.DrnError("detect_all: topk = %d (negative = all, or >= 1), %d box columns for %d classes" % (topk, boxes.shape[1], K))
    if R * K > NMS_MAX_N:
        raise C.DrnError("detect_all: %d x %d entries, at most %d per call are built" % (R, K, NMS_MAX_N))
    boxes = _device_f32(boxes)
    dev = boxes.device
    scores = _device_f32(scores, dev)
    cap = max(R * K, 1)
    nbytes = C.lib().drn_detect_all_workspace_bytes(cap)
    ws = torch.empty((nbytes,), dtype=torch.uint8, device=dev)
    slots = cap if topk < 0 else min(topk, cap)
    ob = torch.empty((slots, 4), dtype=torch.float32, device=dev)
    os_ = torch.empty((slots,), dtype=torch.float32, device=dev)
    oc = torch.empty((slots,), dtype=torch.int32, device=dev)
    orow = torch.empty((slots,), dtype=torch.int32, device=dev)
    nk = torch.empty((1,), dtype=torch.int32, device=dev)
    C.call("drn_detect_all", C.ptr(boxes), C.ptr(scores), R, K, nreg, float(image_shape[0]), float(image_shape[1]),
           float(score_thresh), float(nms_thresh), topk, C.ptr(ws), nbytes, cap, C.ptr(ob), C.ptr(os_), C.ptr(oc), C.ptr(orow),
           C.ptr(nk), C.stream())
    n = int(nk.item())
    return ob[:n], os_[:n], oc[:n].long(), orow[:n].long()


def pairwise_iou(a, b):
    """detectron2.structures.pairwise_iou (boxes.py:329-361) on tensors: a [N, 4], b [M, 4] XYXY -> [N, M] fp32 on the device, the
    fp32 formula of label_proposals / proposal_recall.  An empty N or M launches nothing."""
    if a.dim() != 2 or a.shape[1] != 4 or b.dim() != 2 or b.shape[1] != 4:
        raise C.DrnError("pairwise_iou: boxes [N, 4] and [M, 4] expected, got %s, %s" % (tuple(a.shape), tuple(b.shape)))
    N, M = a.shape[0], b.shape[0]
    if N == 0 or M == 0:
        return torch.empty((N, M), dtype=torch.float32, device=a.device)
    a = _device_f32(a)
    b = _device_f32(b, a.device)
    out = torch.empty((N, M), dtype=torch.float32, device=a.device)
    C.call("drn_pairwise_iou", C.ptr(a), C.ptr(b), N, M, C.ptr(out), C.stream())
    return out


def match(quality, thresholds, labels):
    """Matcher.__call__ (matcher.py:61-103) without low-quality matches (drn_match): quality [N, M] -> (matches [M] int64: the row of
    each column's maximum, the first row on ties; match_labels [M] int8: labels[t] of the interval thresholds[t - 1] <= max <
    thresholds[t]).  thresholds: 1 .. 3 ascending values WITHOUT the infinities, labels one more, each -1 / 0 / 1.  N = 0: matches 0,
    labels[0]."""
    thresholds, labels = [float(t) for t in thresholds], [int(l) for l in labels]
    if quality.dim() != 2 or not 1 <= len(thresholds) <= 3 or len(labels) != len(thresholds) + 1 or any(
            l not in (-1, 0, 1) for l in labels):
        raise C.DrnError("match: quality [N, M], 1 .. 3 thresholds and one label more (each -1, 0 or 1) expected, got %s, %s, %s"
                         % (tuple(quality.shape), thresholds, labels))
    N, M = quality.shape
    if M == 0:
        return (torch.empty((0,), dtype=torch.int64, device=quality.device),
                torch.empty((0,), dtype=torch.int8, device=quality.device))
    quality = _device_f32(quality)
    dev = quality.device
    matches = torch.empty((M,), dtype=torch.int64, device=dev)
    mlab = torch.empty((M,), dtype=torch.int8, device=dev)
    th, lb = C.host_floats(thresholds), C.host_ints(labels)
    C.call("drn_match", C.ptr(quality) if N > 0 else None, N, M, ctypes.cast(th, ctypes.c_void_p), len(thresholds),
           ctypes.cast(lb, ctypes.c_void_p), C.ptr(matches), C.ptr(mlab), C.stream())
    return matches, mlab


DETECT_MAX_IMAGES, DETECT_BATCH_MAX_ENTRIES = 16, 4194304  # include/drn_wsod.h DRN_DETECT_MAX_IMAGES / _BATCH_MAX_ENTRIES


def detect_topk_batch(boxes, scores, img_off, image_sizes, output_sizes=None, *, score_thresh, nms_thresh, topk):
    """The inference tail of all images of a call in one launch chain, without a host read (drn_detect_topk_batch).
    boxes [M, 4*nreg] f32, scores [M, K+1] f32 with the rows of image i contiguous; img_off: N+1 HOST ints; image_sizes: N (h, w) to
    clip to; output_sizes: N (h, w) - detector_postprocess to that size is applied on the device - or None for the raw tail.
    Returns padded device tensors (boxes [N, topk, 4] f32, scores [N, topk] f32, classes [N, topk] i32, rows [N, topk] i32,
    count [N] i32): image i's first count[i] slots are detect_topk (+ detector_postprocess) on its rows, bit for bit; the slots
    beyond hold 0 / 0 / -1 / -1.  More than DETECT_MAX_IMAGES images or DETECT_BATCH_MAX_ENTRIES = M * K entries raise DrnError
    before any launch: callers chunk."""
    if torch.is_tensor(img_off):
        if img_off.is_cuda:
            raise C.DrnError("detect_topk_batch: img_off is known on the host; a device tensor would have to be read back")
        img_off = img_off.tolist()
    off = [int(v) for v in img_off]
    n_img = len(off) - 1
    M, K = scores.shape[0], scores.shape[1] - 1
    nreg = boxes.shape[1] // 4
    if not 1 <= n_img <= DETECT_MAX_IMAGES:
        raise C.DrnError("detect_topk_batch: %d images, 1 .. %d per call are built (chunk the batch)" % (n_img, DETECT_MAX_IMAGES))
    if M * K > DETECT_BATCH_MAX_ENTRIES:
        raise C.DrnError("detect_topk_batch: %d x %d entries, at most %d per call are built (chunk the batch)"
                         % (M, K, DETECT_BATCH_MAX_ENTRIES))
    if not 1 <= int(topk) <= 1024:
        raise C.DrnError("detect_topk_batch: topk = %d, 1 .. 1024 are built" % topk)
    if off[0] != 0 or off[-1] != M or any(b < a for a, b in zip(off[:-1], off[1:])) or boxes.shape[0] != M or K < 1:
        raise C.DrnError("detect_topk_batch: img_off %s does not split %d rows into %d images" % (off, M, n_img))
    if len(image_sizes) != n_img or (output_sizes is not None and len(output_sizes) != n_img):
        raise C.DrnError("detect_topk_batch: one (h, w) per image")
    geom = []
    for i, (h, w) in enumerate(image_sizes):
        oh, ow = output_sizes[i] if output_sizes is not None else (h, w)
        # detector_postprocess forms the scales in double; Boxes.scale rounds them to fp32 once (ctypes does the same here)
        geom += [h, w, oh, ow, ow / w, oh / h]
    dev = boxes.device
    cap = max(M * K, 1)
    nbytes = C.lib().drn_detect_batch_workspace_bytes(cap, n_img)
    ws = torch.empty((nbytes,), dtype=torch.uint8, device=dev)
    boxes = boxes.contiguous().float()
    scores = scores.contiguous().float()
    ob = torch.empty((n_img, topk, 4), dtype=torch.float32, device=dev)
    os_ = torch.empty((n_img, topk), dtype=torch.float32, device=dev)
    oc = torch.empty((n_img, topk), dtype=torch.int32, device=dev)
    orow = torch.empty((n_img, topk), dtype=torch.int32, device=dev)
    cnt = torch.empty((n_img,), dtype=torch.int32, device=dev)
    C.call("drn_detect_topk_batch", C.ptr(boxes), C.ptr(scores), ctypes.cast(C.host_ints(off), ctypes.c_void_p), n_img, K, nreg,
           ctypes.cast(C.host_floats(geom), ctypes.c_void_p), int(output_sizes is not None), float(score_thresh),
           float(nms_thresh), int(topk), C.ptr(ws), nbytes, cap, C.ptr(ob), C.ptr(os_), C.ptr(oc), C.ptr(orow), C.ptr(cnt),
           C.stream())
    return ob, os_, oc, orow, cnt


DETECT_UNION_MAX_BLOCKS = 256  # include/drn_wsod.h DRN_DETECT_UNION_MAX_BLOCKS


def detect_union_batch(boxes, scores, classes, count, img_off, tfms, image_sizes, *, num_classes, score_thresh=1e-8, nms_thresh,
                       topk):
    """GeneralizedRCNNWithTTAUNION's merge for all images of a call in one launch chain, without a host read
    (drn_detect_union_batch).  boxes [B, blk_topk, 4] f32, scores [B, blk_topk] f32, classes [B, blk_topk] i32, count [B] i32: the
    padded blocks of detect_topk_batch, one per augmentation pass; the blocks of image i are img_off[i] .. img_off[i + 1] (N + 1 HOST
    ints); tfms: B (sx, sy, flip_w) of the inverse box transform (sx, sy rounded to float32 like the reference's numpy code);
    image_sizes: N (h, w) of the original images.  Returns the padded tensors of detect_topk_batch (boxes [N, topk, 4], scores,
    classes, rows [N, topk], count [N]); rows index the image's finite union rows in (block, slot) order.  The limits (N <= 16,
    B <= 256, blk_topk and topk <= 1024) raise DrnError before the library is touched."""
    if torch.is_tensor(img_off):
        if img_off.is_cuda:
            raise C.DrnError("detect_union_batch: img_off is known on the host; a device tensor would have to be read back")
        img_off = img_off.tolist()
    off = [int(v) for v in img_off]
    n_img = len(off) - 1
    if scores.dim() != 2:
        raise C.DrnError("detect_union_batch: scores are padded blocks [B, blk_topk]")
    B, blk_topk = scores.shape
    if not 1 <= n_img <= DETECT_MAX_IMAGES:
        raise C.DrnError("detect_union_batch: %d images, 1 .. %d per call are built" % (n_img, DETECT_MAX_IMAGES))
    if not 1 <= B <= DETECT_UNION_MAX_BLOCKS:
        raise C.DrnError("detect_union_batch: %d blocks, 1 .. %d per call are built" % (B, DETECT_UNION_MAX_BLOCKS))
    if not 1 <= blk_topk <= 1024:
        raise C.DrnError("detect_union_batch: blocks of %d slots, 1 .. 1024 are built" % blk_topk)
    if not 1 <= int(topk) <= 1024:
        raise C.DrnError("detect_union_batch: topk = %d, 1 .. 1024 are built" % topk)
    if int(num_classes) < 1:
        raise C.DrnError("detect_union_batch: num_classes = %d" % num_classes)
    if off[0] != 0 or off[-1] != B or any(b < a for a, b in zip(off[:-1], off[1:])):
        raise C.DrnError("detect_union_batch: img_off %s does not split %d blocks into %d images" % (off, B, n_img))
    if tuple(boxes.shape) != (B, blk_topk, 4) or tuple(classes.shape) != (B, blk_topk) or tuple(count.shape) != (B,):
        raise C.DrnError("detect_union_batch: boxes %s / classes %s / count %s do not match scores %s"
                         % (tuple(boxes.shape), tuple(classes.shape), tuple(count.shape), tuple(scores.shape)))
    if boxes.dtype != torch.float32 or scores.dtype != torch.float32 or classes.dtype != torch.int32 or count.dtype != torch.int32:
        raise C.DrnError("detect_union_batch: boxes / scores are float32, classes / count int32")
    if len(tfms) != B or len(image_sizes) != n_img:
        raise C.DrnError("detect_union_batch: one (sx, sy, flip_w) per block and one (h, w) per image")
    tfm = []
    for sx, sy, flip_w in tfms:
        tfm += [np.float32(sx), np.float32(sy), flip_w]
    geom = []
    for h, w in image_sizes:
        geom += [h, w]
    dev = scores.device
    cap = B * blk_topk
    nbytes = C.lib().drn_detect_union_workspace_bytes(cap, n_img)
    ws = torch.empty((nbytes,), dtype=torch.uint8, device=dev)
    boxes, scores, classes, count = boxes.contiguous(), scores.contiguous(), classes.contiguous(), count.contiguous()
    ob = torch.empty((n_img, topk, 4), dtype=torch.float32, device=dev)
    os_ = torch.empty((n_img, topk), dtype=torch.float32, device=dev)
    oc = torch.empty((n_img, topk), dtype=torch.int32, device=dev)
    orow = torch.empty((n_img, topk), dtype=torch.int32, device=dev)
    cnt = torch.empty((n_img,), dtype=torch.int32, device=dev)
    C.call("drn_detect_union_batch", C.ptr(boxes), C.ptr(scores), C.ptr(classes), C.ptr(count), B, blk_topk,
           ctypes.cast(C.host_ints(off), ctypes.c_void_p), n_img, ctypes.cast(C.host_floats(tfm), ctypes.c_void_p),
           ctypes.cast(C.host_floats(geom), ctypes.c_void_p), int(num_classes), float(score_thresh), float(nms_thresh), int(topk),
           C.ptr(ws), nbytes, cap, C.ptr(ob), C.ptr(os_), C.ptr(oc), C.ptr(orow), C.ptr(cnt), C.stream())
    return ob, os_, oc, orow, cnt


def detections_compact(boxes, scores, classes, count, image_index):
    """Padded blocks -> packed detections on the device (drn_detect_compact): boxes [B, topk, 4] f32, scores [B, topk] f32,
    classes [B, topk] i32, count [B] i32, image_index [B] i32 -> (boxes [B*topk, 4], scores, classes, images [B*topk], n [1] i32):
    the first n rows are the live slots in block order then slot order, the rows beyond are zero.  No host read: n stays on the
    device."""
    B, topk = scores.shape[0], scores.shape[1]
    dev = scores.device
    assert boxes.shape == (B, topk, 4) and classes.shape == (B, topk) and count.shape == (B,) and image_index.shape == (B,)
    assert boxes.dtype == torch.float32 and scores.dtype == torch.float32
    assert classes.dtype == torch.int32 and count.dtype == torch.int32 and image_index.dtype == torch.int32
    boxes, scores, classes = boxes.contiguous(), scores.contiguous(), classes.contiguous()
    count, image_index = count.contiguous(), image_index.contiguous()
    ob = torch.zeros((B * topk, 4), dtype=torch.float32, device=dev)
    os_ = torch.zeros((B * topk,), dtype=torch.float32, device=dev)
    oc = torch.zeros((B * topk,), dtype=torch.int32, device=dev)
    oi = torch.zeros((B * topk,), dtype=torch.int32, device=dev)
    offs = torch.empty((B + 1,), dtype=torch.int32, device=dev)
    n = torch.empty((1,), dtype=torch.int32, device=dev)
    C.call("drn_detect_compact", C.ptr(boxes), C.ptr(scores), C.ptr(classes), C.ptr(count), C.ptr(image_index), B, max(topk, 1),
           C.ptr(offs), C.ptr(ob), C.ptr(os_), C.ptr(oc), C.ptr(oi), C.ptr(n), C.stream())
    return ob, os_, oc, oi, n


def tta_accumulate(boxes, scores, acc_boxes, acc_scores, sx, sy, flip_w, first, n_final):
    """fold one augmentation's [R, 4K] boxes / [R, K+1] scores into the running TTA averages (see the header)"""
    assert boxes.is_contiguous() and scores.is_contiguous() and boxes.dtype == torch.float32 and scores.dtype == torch.float32
    assert acc_boxes.shape == boxes.shape and acc_scores.shape == scores.shape
    C.call("drn_tta_accumulate", C.ptr(boxes), C.ptr(scores), C.ptr(acc_boxes), C.ptr(acc_scores), boxes.numel() // 4,
           scores.numel(), float(sx), float(sy), float(flip_w), int(first), int(n_final), C.stream())


def pcl_adjacency(boxes, iou_thr=0.4):
    """[R, ceil(R/32)] uint32 bit matrix of IoU(boxes, boxes) > iou_thr (third_party/pcl.py:78-87)"""
    R = boxes.shape[0]
    assert boxes.dtype == torch.float32 and boxes.is_contiguous()
    adj = torch.empty((R, (R + 31) // 32), dtype=torch.int32, device=boxes.device)
    C.call("drn_pcl_adjacency", C.ptr(boxes), R, float(iou_thr), C.ptr(adj), C.stream())
    return adj


def pcl_refine(logits, col0s, K, wsddn_scores, boxes, adj, onehot, dlogits):
    """PCL targets + loss + d loss / d logits of every refinement branch of ONE image (see include/drn_wsod.h).
    Returns a list of per-branch dicts (targets, clusters, probs, loss view)."""
    R, dev, nb = boxes.shape[0], boxes.device, len(col0s)
    pmax = min(640, 5 * K)
    e = lambda shape, dt: torch.empty(shape, dtype=dt, device=dev)
    probs = e((nb, R, K + 1), torch.float32)
    row = dict(labels=e((nb, R), torch.int32), cls_loss_weights=e((nb, R), torch.float32),
               gt_assignment=e((nb, R), torch.int32))
    pc = dict(pc_labels=e((nb, pmax), torch.int32), pc_probs=e((nb, pmax), torch.float32),
              pc_count=e((nb, pmax), torch.int32), img_cls_loss_weights=e((nb, pmax), torch.float32),
              pc_rows=e((nb, pmax), torch.int32), pc_scores=e((nb, pmax), torch.float32))
    n_pc = e((nb,), torch.int32)
    losses = e((nb,), torch.float32)
    c0 = C.host_ints(col0s)
    C.call("drn_pcl_refine", C.ptr(logits), _2d(logits), ctypes.cast(c0, ctypes.c_void_p), nb, K, C.ptr(wsddn_scores),
           _2d(wsddn_scores), C.ptr(boxes), C.ptr(adj), C.ptr(onehot), R, C.ptr(probs),
           C.ptr(row["labels"]), C.ptr(row["cls_loss_weights"]), C.ptr(row["gt_assignment"]), C.ptr(pc["pc_labels"]),
           C.ptr(pc["pc_probs"]), C.ptr(pc["pc_count"]), C.ptr(pc["img_cls_loss_weights"]), C.ptr(pc["pc_rows"]),
           C.ptr(pc["pc_scores"]), C.ptr(n_pc), pmax, C.ptr(losses), C.ptr(dlogits), C.stream())
    out = []
    for b in range(nb):
        d = {k: v[b] for k, v in row.items()}
        d.update({k: v[b] for k, v in pc.items()})
        d.update(n_pc=n_pc[b: b + 1], probs=probs[b], loss=losses[b: b + 1])
        out.append(d)
    return out


PCL_MAX_IMAGES, PCL_MAX_ROWS = 16, 4096  # include/drn_wsod.h DRN_PCL_MAX_IMAGES, the per-image limit of the PCL entries


def _pcl_img_off(img_off, n_img, M, max_rows, dev):
    """img_off of a PCL batch on the device.  A HOST tensor (or list) is checked first, where the sizes are known: ascending
    from 0 to M, every image within 1 .. max_rows - refused without a launch - and then uploaded.  A device tensor is taken as
    it is (no read-back): the kernels skip an image outside max_rows and make its loss NaN."""
    if not 1 <= int(n_img) <= PCL_MAX_IMAGES:
        raise C.DrnError("PCL image batch: %d images, 1 .. %d are built" % (n_img, PCL_MAX_IMAGES))
    if not 1 <= int(max_rows) <= PCL_MAX_ROWS:
        raise C.DrnError("PCL image batch: max_rows = %d, 1 .. %d proposals per image are built" % (max_rows, PCL_MAX_ROWS))
    if not torch.is_tensor(img_off):
        img_off = torch.tensor(list(img_off), dtype=torch.int32)
    assert img_off.dtype == torch.int32 and img_off.numel() == n_img + 1 and img_off.is_contiguous()
    if not img_off.is_cuda:
        o = img_off.tolist()
        rows = [b - a for a, b in zip(o[:-1], o[1:])]
        if o[0] != 0 or o[-1] != M or min(rows) < 1:
            raise C.DrnError("PCL image batch: img_off %s does not split %d rows into %d non-empty images" % (o, M, n_img))
        if max(rows) > max_rows:
            raise C.DrnError("PCL image batch: an image has %d proposals, max_rows = %d" % (max(rows), max_rows))
        img_off = img_off.to(dev)
    return img_off


def pcl_adjacency_batch(boxes, img_off, n_img, max_rows, iou_thr=0.4):
    """[M, ceil(max_rows/32)] uint32: per image the bit matrix of pcl_adjacency, bit columns local to the image, zero beyond
    its row count (drn_pcl_adjacency_batch).  img_off int32 [n_img + 1]: device tensor, or host tensor (checked, see above)."""
    M = boxes.shape[0]
    assert boxes.dtype == torch.float32 and boxes.is_contiguous()
    img_off = _pcl_img_off(img_off, n_img, M, max_rows, boxes.device)
    adj = torch.empty((M, (int(max_rows) + 31) // 32), dtype=torch.int32, device=boxes.device)
    C.call("drn_pcl_adjacency_batch", C.ptr(boxes), C.ptr(img_off), int(n_img), M, int(max_rows), float(iou_thr), C.ptr(adj),
           C.stream())
    return adj


def pcl_refine_batch(logits, col0s, K, wsddn_scores, boxes, adj, onehot, img_off, n_img, max_rows, dlogits, rows=None):
    """pcl_refine for every image of a batch in one launch of (branch, image) workgroups (see include/drn_wsod.h: per image
    bit for bit the single-image results, batch loss = mean over images in ascending order, dlogits * 1 / n_img).
    onehot [n_img, K]; adj from pcl_adjacency_batch with the same max_rows.  Returns (per_image, loss_img [n_img, NB],
    loss [NB]): per_image[i][b] is the dict pcl_refine returns for image i alone - views of the batch's buffers, cut at the
    image's rows when the host knows them (img_off on the host, or rows = the per-image counts); `loss` in it is loss_img[i, b]."""
    M, dev, nb = boxes.shape[0], boxes.device, len(col0s)
    if rows is None and torch.is_tensor(img_off) and not img_off.is_cuda:
        o = img_off.tolist()
        rows = [b - a for a, b in zip(o[:-1], o[1:])]
    img_off = _pcl_img_off(img_off, n_img, M, max_rows, dev)
    assert adj.shape == (M, (int(max_rows) + 31) // 32) and adj.is_contiguous()
    assert onehot.shape == (n_img, K) and onehot.dtype == torch.float32 and onehot.is_contiguous()
    pmax = min(640, 5 * K)
    e = lambda shape, dt: torch.empty(shape, dtype=dt, device=dev)
    probs = e((nb, M, K + 1), torch.float32)
    row = dict(labels=e((nb, M), torch.int32), cls_loss_weights=e((nb, M), torch.float32),
               gt_assignment=e((nb, M), torch.int32))
    pc = dict(pc_labels=e((n_img, nb, pmax), torch.int32), pc_probs=e((n_img, nb, pmax), torch.float32),
              pc_count=e((n_img, nb, pmax), torch.int32), img_cls_loss_weights=e((n_img, nb, pmax), torch.float32),
              pc_rows=e((n_img, nb, pmax), torch.int32), pc_scores=e((n_img, nb, pmax), torch.float32))
    n_pc = e((n_img, nb), torch.int32)
    loss_img = e((n_img, nb), torch.float32)
    losses = e((nb,), torch.float32)
    c0 = C.host_ints(col0s)
    C.call("drn_pcl_refine_batch", C.ptr(logits), _2d(logits), ctypes.cast(c0, ctypes.c_void_p), nb, K, C.ptr(wsddn_scores),
           _2d(wsddn_scores), C.ptr(boxes), C.ptr(adj), C.ptr(onehot), C.ptr(img_off), int(n_img), M, int(max_rows),
           C.ptr(probs), C.ptr(row["labels"]), C.ptr(row["cls_loss_weights"]), C.ptr(row["gt_assignment"]),
           C.ptr(pc["pc_labels"]), C.ptr(pc["pc_probs"]), C.ptr(pc["pc_count"]), C.ptr(pc["img_cls_loss_weights"]),
           C.ptr(pc["pc_rows"]), C.ptr(pc["pc_scores"]), C.ptr(n_pc), pmax, C.ptr(loss_img), C.ptr(losses), C.ptr(dlogits),
           C.stream())
    per_image, r0 = [], 0
    for i in range(n_img):
        sl = slice(None) if rows is None else slice(r0, r0 + rows[i])
        out = []
        for b in range(nb):
            d = {k: v[b, sl] for k, v in row.items()}
            d.update({k: v[i, b] for k, v in pc.items()})
            d.update(n_pc=n_pc[i, b: b + 1], probs=probs[b, sl], loss=loss_img[i, b: b + 1])
            out.append(d)
        per_image.append(out)
        r0 += 0 if rows is None else rows[i]
    return per_image, loss_img, losses


COCO_MAX_GT, COCO_MAX_AREAS, COCO_MAX_REC = 512, 4, 128  # include/drn_wsod.h DRN_COCO_MAX_*


def _coco_ws_bytes(n, segments):
    """DRN_COCO_WS_BYTES of include/drn_wsod.h"""
    return 40 * (n + 4) + 8192 * ((n + 4095) // 4096 + 1) + 32 * segments + 1024


def coco_match(det_box, det_score, det_pair, gt_box, gt_area, gt_crowd, gt_off, num_cats, max_gt, iou_thr, area_rng,
               max_det=100, stages=3, out=None):
    """COCO per-(image, category) matching (see include/drn_wsod.h, drn_coco_match).  det_box [n, 4] f64 XYWH, det_score
    [n] f32, det_pair [n] i32 = image index * num_cats + category index; gt_box [G, 4] f64, gt_area [G] f64, gt_crowd [G]
    u8, gt_off [P + 1] i32, all on the device; max_gt = most GT of one pair (a host number).  Returns a dict: order,
    s_score, s_cat, s_rank, dm, di (int64 tensors holding the 64-bit words), npig [P, A], gt_ign [G].  stages = 1 / 2
    with out = the dict of the stages = 1 call runs the ordering and the matching apart."""
    dev = det_box.device
    n, P, T, A = det_score.shape[0], gt_off.shape[0] - 1, iou_thr.shape[0], area_rng.shape[0]
    assert det_box.dtype == torch.float64 and det_box.is_contiguous() and det_box.shape == (n, 4)
    assert det_score.dtype == torch.float32 and det_pair.dtype == torch.int32 and det_pair.shape[0] == n
    assert gt_box.dtype == torch.float64 and gt_area.dtype == torch.float64 and gt_crowd.dtype == torch.uint8
    assert gt_off.dtype == torch.int32 and iou_thr.dtype == torch.float64 and area_rng.dtype == torch.float64
    assert gt_box.is_contiguous() and area_rng.is_contiguous() and area_rng.shape == (A, 2) and P % num_cats == 0
    G = gt_area.shape[0]
    if out is None:
        e = lambda shape, dt: torch.empty(shape, dtype=dt, device=dev)
        nbytes = _coco_ws_bytes(n, P)
        out = dict(ws=e((nbytes,), torch.uint8), order=e((n,), torch.int32), s_score=e((n,), torch.float32),
                   s_cat=e((n,), torch.int32), s_rank=e((n,), torch.int32), dm=e((n,), torch.int64),
                   di=e((n,), torch.int64), npig=e((P, A), torch.int32), gt_ign=e((G,), torch.uint8))
    o = out
    C.call("drn_coco_match", C.ptr(det_box), C.ptr(det_score), C.ptr(det_pair), n, C.ptr(gt_box), C.ptr(gt_area),
           C.ptr(gt_crowd), C.ptr(gt_off), P, int(num_cats), int(max_gt), C.ptr(iou_thr), T, C.ptr(area_rng), A,
           int(max_det), C.ptr(o["ws"]), o["ws"].numel(), int(stages), C.ptr(o["order"]), C.ptr(o["s_score"]),
           C.ptr(o["s_cat"]), C.ptr(o["s_rank"]), C.ptr(o["dm"]), C.ptr(o["di"]), C.ptr(o["npig"]), C.ptr(o["gt_ign"]),
           C.stream())
    return out


def coco_accumulate(s_score, s_cat, s_rank, dm, di, npig, num_images, num_cats, num_iou, max_dets, rec_thr, stages=3,
                    out=None):
    """COCO precision / recall accumulation (drn_coco_accumulate) over the records coco_match returns.  npig [I * K, A]
    i32, max_dets [M] i32, rec_thr [R] f64 on the device.  Returns a dict with precision / scores [T, R, K, A, M] and
    recall [T, K, A, M] (f64, -1 where a category has no countable GT)."""
    dev = npig.device
    n, A, M, R, T, K = s_score.shape[0], npig.shape[1], max_dets.shape[0], rec_thr.shape[0], int(num_iou), int(num_cats)
    assert s_score.dtype == torch.float32 and s_cat.dtype == torch.int32 and s_rank.dtype == torch.int32
    assert dm.dtype == torch.int64 and di.dtype == torch.int64 and npig.dtype == torch.int32 and npig.is_contiguous()
    assert max_dets.dtype == torch.int32 and rec_thr.dtype == torch.float64 and npig.shape[0] == num_images * K
    assert s_cat.shape[0] == n and s_rank.shape[0] == n and dm.shape[0] == n and di.shape[0] == n
    if out is None:
        e = lambda shape, dt: torch.empty(shape, dtype=dt, device=dev)
        out = dict(ws=e((_coco_ws_bytes(n, K),), torch.uint8), precision=e((T, R, K, A, M), torch.float64),
                   scores=e((T, R, K, A, M), torch.float64), recall=e((T, K, A, M), torch.float64))
    o = out
    C.call("drn_coco_accumulate", C.ptr(s_score), C.ptr(s_cat), C.ptr(s_rank), C.ptr(dm), C.ptr(di), n, C.ptr(npig),
           int(num_images), K, T, A, C.ptr(max_dets), M, C.ptr(rec_thr), R, C.ptr(o["ws"]), o["ws"].numel(), int(stages),
           C.ptr(o["precision"]), C.ptr(o["scores"]), C.ptr(o["recall"]), C.stream())
    return out


PROPOSAL_MAX_GT, PROPOSAL_MAX_PER_IMAGE = 256, 4096  # include/drn_wsod.h DRN_PROPOSAL_MAX_*


def proposal_recall(prop_box, prop_logit, prop_off, gt_box, gt_area, gt_off, area_rng, limits, thresholds, max_gt, max_prop,
                    stages=3, out=None):
    """Box-proposal recall matching (see include/drn_wsod.h, drn_proposal_recall).  prop_box [P, 4] f32 XYXY, prop_logit
    [P] f32, prop_off [I + 1] i32: the images' proposals, concatenated; gt_box [G, 4] f32 XYXY, gt_area [G] f32, gt_off
    [I + 1] i32: the ground truth that is not crowd, in annotation order; area_rng [A, 2] f32, limits [L] i32 (<= 0: no
    cut), thresholds [T] f32 - all on the device.  max_gt / max_prop = most boxes of one image / most proposals of one image
    after the cut (host numbers).  Returns a dict: overlaps [A, L, G] f32 (-1 = not an entry), counts [A, L, T] and num_pos
    [A] (int64).  stages = 1 / 2 with out = the dict of the stages = 1 call runs the ordering and the matching apart."""
    dev = prop_box.device
    P, G, I = prop_logit.shape[0], gt_area.shape[0], gt_off.shape[0] - 1
    A, L, T = area_rng.shape[0], limits.shape[0], thresholds.shape[0]
    assert prop_box.dtype == torch.float32 and prop_box.is_contiguous() and prop_box.shape == (P, 4)
    assert prop_logit.dtype == torch.float32 and prop_logit.is_contiguous()
    assert prop_off.dtype == torch.int32 and prop_off.shape == (I + 1,) and prop_off.is_contiguous()
    assert gt_box.dtype == torch.float32 and gt_box.is_contiguous() and gt_box.shape == (G, 4)
    assert gt_area.dtype == torch.float32 and gt_area.is_contiguous()
    assert gt_off.dtype == torch.int32 and gt_off.is_contiguous() and I >= 1
    assert area_rng.dtype == torch.float32 and area_rng.is_contiguous() and area_rng.shape == (A, 2)
    assert limits.dtype == torch.int32 and limits.is_contiguous() and limits.dim() == 1
    assert thresholds.dtype == torch.float32 and thresholds.is_contiguous() and thresholds.dim() == 1
    if out is None:
        e = lambda shape, dt: torch.empty(shape, dtype=dt, device=dev)
        nbytes = int(C.lib().drn_proposal_recall_workspace_bytes(P))
        out = dict(ws=e((nbytes,), torch.uint8), overlaps=e((A, L, G), torch.float32), counts=e((A, L, T), torch.int64),
                   num_pos=e((A,), torch.int64))
    o = out
    C.call("drn_proposal_recall", C.ptr(prop_box), C.ptr(prop_logit), C.ptr(prop_off), P, C.ptr(gt_box), C.ptr(gt_area),
           C.ptr(gt_off), G, I, int(max_gt), int(max_prop), C.ptr(area_rng), A, C.ptr(limits), L, C.ptr(thresholds), T,
           C.ptr(o["ws"]), o["ws"].numel(), int(stages), C.ptr(o["overlaps"]), C.ptr(o["counts"]), C.ptr(o["num_pos"]),
           C.stream())
    return out


VOC_MAX_GT, VOC_MAX_REC = 128, 16  # include/drn_wsod.h DRN_VOC_MAX_*


def _voc_ws_bytes(n, pairs):
    """DRN_VOC_WS_BYTES of include/drn_wsod.h"""
    return 24 * (n + 4) + 8192 * ((n + 4095) // 4096 + 1) + 4 * pairs + 1024


def voc_match(det_box, det_score, det_pair, gt_box, gt_diff, gt_off, num_classes, max_gt, iou_thr, stages=3, out=None):
    """PASCAL VOC ranking and matching (see include/drn_wsod.h, drn_voc_match).  det_box [n, 4] f32 XYXY as predicted,
    det_score [n] f32, det_pair [n] i32 = image index * num_classes + class, in processing order; gt_box [G, 4] f64,
    gt_diff [G] u8, gt_off [P + 1] i32, iou_thr [T] f64, all on the device; max_gt = most GT of one pair (a host number).
    Returns a dict in rank order (class, descending quantised score, processing order on ties): order, s_score, ovmax,
    jmax, tp / fp (int64 tensors holding the 64-bit words, bit t = threshold t), plus cls_off [K + 1] and hit [P].
    stages = 1 / 2 with out = the dict of the stages = 1 call runs the ranking and the matching apart."""
    dev = det_box.device
    n, P, T = det_score.shape[0], gt_off.shape[0] - 1, iou_thr.shape[0]
    K = int(num_classes)
    assert det_box.dtype == torch.float32 and det_box.is_contiguous() and det_box.shape == (n, 4)
    assert det_score.dtype == torch.float32 and det_pair.dtype == torch.int32 and det_pair.shape[0] == n
    assert det_score.is_contiguous() and det_pair.is_contiguous() and gt_box.is_contiguous()
    assert gt_box.dtype == torch.float64 and gt_diff.dtype == torch.uint8 and gt_box.shape == (gt_diff.shape[0], 4)
    assert gt_off.dtype == torch.int32 and iou_thr.dtype == torch.float64 and P % K == 0
    if out is None:
        e = lambda shape, dt: torch.empty(shape, dtype=dt, device=dev)
        out = dict(ws=e((_voc_ws_bytes(n, P),), torch.uint8), order=e((n,), torch.int32), s_score=e((n,), torch.float64),
                   cls_off=e((K + 1,), torch.int32), ovmax=e((n,), torch.float64), jmax=e((n,), torch.int32),
                   tp=e((n,), torch.int64), fp=e((n,), torch.int64), hit=e((P,), torch.int64))
    o = out
    C.call("drn_voc_match", C.ptr(det_box), C.ptr(det_score), C.ptr(det_pair), n, C.ptr(gt_box), C.ptr(gt_diff),
           C.ptr(gt_off), P, K, int(max_gt), C.ptr(iou_thr), T, C.ptr(o["ws"]), o["ws"].numel(), int(stages),
           C.ptr(o["order"]), C.ptr(o["s_score"]), C.ptr(o["cls_off"]), C.ptr(o["ovmax"]), C.ptr(o["jmax"]), C.ptr(o["tp"]),
           C.ptr(o["fp"]), C.ptr(o["hit"]), C.stream())
    return out


def voc_accumulate(tp, fp, cls_off, hit, npos, npos_im, num_iou, rec_thr, use_07_metric, curve_at=None):
    """PASCAL VOC AP and CorLoc (drn_voc_accumulate) over the records voc_match returns.  npos / npos_im [K] i32 and
    rec_thr [R] f64 (np.arange(0.0, 1.1, 0.1); read by the VOC07 metric only) on the device.  Returns a dict with ap and
    corloc [T, K] f64 and, with curve_at = a threshold index, rec / prec [n] of that threshold in rank order."""
    dev = cls_off.device
    n, K, T, R = tp.shape[0], cls_off.shape[0] - 1, int(num_iou), rec_thr.shape[0]
    assert tp.dtype == torch.int64 and fp.dtype == torch.int64 and hit.dtype == torch.int64 and fp.shape[0] == n
    assert cls_off.dtype == torch.int32 and npos.dtype == torch.int32 and npos_im.dtype == torch.int32
    assert npos.shape[0] == K and npos_im.shape[0] == K and rec_thr.dtype == torch.float64 and hit.shape[0] % K == 0
    e = lambda shape: torch.empty(shape, dtype=torch.float64, device=dev)
    out = dict(ap=e((T, K)), corloc=e((T, K)))
    if curve_at is not None:
        out.update(rec=e((n,)), prec=e((n,)))
    C.call("drn_voc_accumulate", C.ptr(tp), C.ptr(fp), n, C.ptr(cls_off), C.ptr(hit), C.ptr(npos), C.ptr(npos_im),
           hit.shape[0] // K, K, T, C.ptr(rec_thr), R, int(bool(use_07_metric)), -1 if curve_at is None else int(curve_at),
           C.ptr(out["ap"]), C.ptr(out["corloc"]), C.ptr(out.get("rec")), C.ptr(out.get("prec")), C.stream())
    return out
