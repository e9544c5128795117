"""The heads' loss and reduction kernels against fp64 references: box regression loss, the two-stage column sums of the
bias gradients (also through split-K grad_out), sum_small, the mean of the refinement softmaxes, the OICR cross entropy
and the counter-based dropout masks as the training step draws them.

Every input is built on the CPU from a fixed seed.  Bounds come from the arithmetic: u = 2^-24, an fp32 sum of n terms in
any order is within gamma_n * sum|x_i| of the exact one, gamma_n = n u / (1 - n u).  Output buffers are larger than the
region an op owns and pre-filled with a sentinel (NaN or 7.0); the tests check that it survives outside that region.
Input buffers carry NaN outside the region an op may read, so an over-read shows up as a NaN result."""
import ctypes
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import golden_util as G
from __graft_entry__ import load_package
from mil_ref_util import softmax_rel_bound as _softmax_rel_bound  # (C + 2 R + 16) u: shared with the MIL loss tests

pytestmark = pytest.mark.gpu
O = G.O
DEV = "cuda"
U = 2.0 ** -24
NAN = float("nan")


def gamma(n):
    return n * U / (1 - n * U)


@pytest.fixture(scope="module")
def drn():
    assert torch.cuda.is_available(), "GPU tests need a GPU (run with -m gpu on the MI355X box)"
    pkg = load_package()
    pkg._cabi.lib()  # raises if the HIP library is missing: no fallback
    import importlib

    return importlib.import_module("drn_wsod_pytorch_amd.ops")


@pytest.fixture(scope="module")
def cabi(drn):
    import importlib

    return importlib.import_module("drn_wsod_pytorch_amd._cabi")


def _f32(x):
    return float(np.float32(x))


def _untouched(buf, region, sentinel):
    """every element of buf outside the boolean region still holds the sentinel"""
    rest = buf.cpu()[~region]
    if math.isnan(sentinel):
        return bool(torch.isnan(rest).all())
    return bool((rest == sentinel).all())


def _region(shape, rows, cols):
    r = torch.zeros(shape, dtype=torch.bool)
    r[rows, cols] = True
    return r


# ------------------------------------------------------------------------------------------- box_reg_loss
def _boxes(rs, M):
    """x0, y0 in [0, 600); widths and heights from exp(U(-1, 7)): aspect ratios up to e^8 either way"""
    xy = rs.uniform(0, 600, (M, 2))
    wh = np.exp(rs.uniform(-1, 7, (M, 2)))
    return torch.from_numpy(np.concatenate([xy, xy + wh], 1).astype(np.float32))


def _exact_rows(props, gt, logits, col0, labels, rows, w32):
    """rows whose fp32 target is exact (integer corners, power-of-two widths, tw == sw: log 1 = 0) and whose prediction
    equals it: |pred - target| = 0 in fp32 and in fp64"""
    for i in rows:
        x0, y0 = float(10 + 3 * (i % 50)), float(20 + (i % 31))
        props[i] = torch.tensor([x0, y0, x0 + 32, y0 + 64])
        gt[i] = torch.tensor([x0 + 4, y0 - 8, x0 + 36, y0 + 56])
        c = col0 + 4 * int(labels[i])
        logits[i, c: c + 4] = torch.tensor([w32[0] * 4 / 32, w32[1] * -8 / 64, 0.0, 0.0])


@pytest.mark.parametrize("K", [5, 20, 80])
@pytest.mark.parametrize("M", [1, 255, 256, 257, 2000, 4099])
def test_box_reg_loss(drn, cabi, M, K):
    """drn_box_reg_loss (loss_box_reg_r{k}: fast_rcnn.py:1146-1211) against oicr_box_reg_loss on fp64 inputs and its autograd
    gradient; partial-block sums of 1, 2 and 17 blocks; deltas at col0 > 0 of a wider row, dlogits with another pitch"""
    rs = np.random.RandomState(1000 * K + M)
    col0, ld, ld_d = 3, 4 * K + 11, 4 * K + 6
    weights = (10.0, 10.0, 5.0, 5.0) if M % 2 else (7.3, 3.1, 2.2, 0.9)
    w32 = tuple(_f32(w) for w in weights)  # the kernel's fp32 weights: the reference uses the same values
    scale = 0.37
    logits = torch.full((M + 1, ld), NAN)  # NaN outside the head's 4K columns and below row M
    logits[:M, col0: col0 + 4 * K] = torch.from_numpy(rs.standard_normal((M, 4 * K)).astype(np.float32) * 2)
    labels = torch.from_numpy(rs.randint(-1, K + 1, M).astype(np.int32))  # foreground, background (= K), ignore (-1)
    # the first and the last partial block hold a foreground row whose loss (~20000 / M) stands well above the bound
    # (gamma_n sum|t| is ~0.7 at M = 4099: the extreme boxes' targets reach 1e4): a combine that drops a block fails
    labels[0] = labels[-1] = int(rs.randint(0, K))
    for i in (0, M - 1):
        logits[i, col0 + 4 * int(labels[i]): col0 + 4 * int(labels[i]) + 4] += 5000.0
    props, gt = _boxes(rs, M), _boxes(rs, M)
    fg = ((labels >= 0) & (labels < K)).nonzero().view(-1)
    exact = [e for e in fg[1::23].tolist() if e != M - 1]
    _exact_rows(props, gt, logits, col0, labels, exact, w32)

    # fp64 reference: the oracle on .double() inputs, autograd for the gradient
    cfg = O.OracleCfg(bbox_weights=w32)
    d64 = logits[:M, col0: col0 + 4 * K].double().requires_grad_(True)
    L64 = O.oicr_box_reg_loss(d64, labels.long(), props.double(), gt.double(), K, cfg)
    L64.backward()
    # error of the kernel's fp32 targets: the same IEEE operations as torch's fp32 ones but for logf (<= 1 ulp on either
    # side, then the weight's multiply): |d32 - d64| + 6 u |d| per target
    t64 = O.get_deltas(props.double(), gt.double(), w32)
    t32 = O.get_deltas(props, gt, w32).double()
    cols = 4 * labels.long()[fg][:, None] + torch.arange(4)
    pred = d64.detach()[fg[:, None], cols]
    diff = pred - t64[fg]
    eps = (t32[fg] - t64[fg]).abs() + 6 * U * t64[fg].abs()
    t = diff.abs()
    n = max(int(t.numel()), 1)
    L64 = float(L64.detach())
    bound = ((eps * (1 + U) + U * t).sum() + gamma(n) * (t + 2 * eps).sum()) / M + 2 * U * abs(L64)

    lgd, labd, propd, gtd = logits.to(DEV), labels.to(DEV), props.to(DEV), gt.to(DEV)
    for with_d in (True, False):
        nb = (M + 255) // 256
        loss = torch.full((2,), NAN, device=DEV)
        scratch = torch.full((nb + 3,), NAN, device=DEV)  # NaN past the nb partials: a combine that reads on gives NaN
        dl = torch.full((M + 1, ld_d), NAN, device=DEV) if with_d else None
        w = cabi.host_floats(weights)
        cabi.call("drn_box_reg_loss", cabi.ptr(lgd), ld, col0, K, cabi.ptr(labd), cabi.ptr(propd), cabi.ptr(gtd),
                  ctypes.cast(w, ctypes.c_void_p), cabi.ptr(dl), ld_d if with_d else 0, cabi.ptr(loss), cabi.ptr(scratch), M,
                  float(scale), cabi.stream())
        lc = loss.cpu()
        assert math.isnan(float(lc[1]))
        assert abs(float(lc[0]) - L64) <= bound, (float(lc[0]), L64, float(bound))
        if not with_d:
            continue
        dlc = dl.cpu()
        win = _region(dl.shape, slice(0, M), slice(col0, col0 + 4 * K))
        assert _untouched(dl, win, NAN)
        got = dlc[:M, col0: col0 + 4 * K]
        # sign(diff) / M * scale in fp32 in the owned columns, exact zeros elsewhere in the window
        sc32 = torch.tensor(scale, dtype=torch.float32)
        g = float(torch.ones((), dtype=torch.float32) / M * sc32)
        ref = d64.grad.sign().float() / M * sc32
        owned = torch.zeros_like(got, dtype=torch.bool)
        owned[fg[:, None], cols] = True
        assert bool((got[~owned] == 0).all())
        gf = got[fg[:, None], cols]
        rf = ref[fg[:, None], cols]
        far = diff.abs() > eps  # the fp32 sign is the fp64 one
        assert torch.equal(gf[far], rf[far])
        assert bool(((gf[~far] == g) | (gf[~far] == -g) | (gf[~far] == 0)).all())
        if exact:  # prediction == target: sign 0, as torch.abs's gradient at 0
            ei = torch.tensor([int((fg == e).nonzero()) for e in exact])
            assert bool((gf[ei] == 0).all()) and bool((rf[ei] == 0).all())


@pytest.mark.parametrize("K", [5, 80])
def test_box_reg_loss_no_foreground(drn, K):
    """a batch with background / ignored rows only: loss exactly 0, the whole dlogits window exactly 0"""
    rs = np.random.RandomState(7 + K)
    M, col0, ld = 300, 2, 4 * K + 5
    logits = torch.from_numpy(rs.standard_normal((M, ld)).astype(np.float32)).to(DEV)
    labels = torch.from_numpy(np.where(rs.rand(M) < 0.5, -1, K).astype(np.int32)).to(DEV)
    props, gt = _boxes(rs, M).to(DEV), _boxes(rs, M).to(DEV)
    dl = torch.full((M, ld + 3), NAN, device=DEV)
    loss = drn.box_reg_loss(logits, col0, K, labels, props, gt, dlogits=dl, loss_scale=2.5)
    assert float(loss) == 0.0
    win = _region(dl.shape, slice(0, M), slice(col0, col0 + 4 * K))
    assert bool((dl.cpu()[win] == 0).all()) and _untouched(dl, win, NAN)


# ------------------------------------------------------------------------------------------- two-stage column sums
def _bwd_case(rs, M, N, S, mode, dtype, colidx):
    """inputs of drn_bias_act_bwd(_splits) in padded buffers, and the kernel's fp32 gradient emulated on the CPU"""
    ldg = (N + 3) // 4 * 4 + 4
    parts = torch.full((S, M + 2, ldg), NAN)
    parts[:, :M, :N] = torch.from_numpy(rs.standard_normal((S, M, N)).astype(np.float32) * np.exp(rs.uniform(-3, 3, (1, 1, N))).astype(np.float32))
    ldo = (N + 3) // 4 * 4 + 4
    saved = torch.zeros((M + 1, ldo))
    saved[:M, :N] = torch.from_numpy(rs.standard_normal((M, N)).astype(np.float32))
    saved[:M, :N][torch.from_numpy(rs.rand(M, N) < 0.1)] = 0.0
    saved = saved.to(dtype)
    mask, drop_p = None, 0.0
    if mode == "mask":
        mask = torch.from_numpy((rs.rand(M, N) > 0.4).astype(np.float32) * np.float32(1 / 0.6))
        mult = mask
    else:
        drop_p = 0.3
        mult = torch.full((M, N), 1.0) / (torch.tensor(1.0) - torch.tensor(drop_p, dtype=torch.float32))
    mult = torch.where(saved[:M, :N].float() > 0, mult, torch.zeros(()))
    if colidx:
        L = 7
        cs_tab = torch.from_numpy(rs.uniform(0.1, 2.0, L).astype(np.float32))
        idx = torch.from_numpy(rs.randint(-1, L, N).astype(np.int32))
        cs = torch.where(idx >= 0, cs_tab[idx.clamp(min=0).long()], torch.zeros(()))
    else:
        cs_tab = torch.from_numpy(rs.uniform(0.1, 2.0, N).astype(np.float32))
        idx, cs = None, cs_tab
    v = parts[0, :M, :N].clone()
    for s in range(1, S):
        v = v + parts[s, :M, :N]
    v32 = (v * cs) * mult  # split partials in order, then the column scale, then the activation / dropout multiplier
    # fp64 reference gradient and sum|.| of its terms (the error of the split sum and both products is inside gamma_{M+S+1})
    p64 = parts[:, :M, :N].double()
    g64 = p64.sum(0) * cs.double() * mult.double()
    mag = p64.abs().sum(0) * cs.double() * mult.double()
    return dict(parts=parts, ldg=ldg, saved=saved, ldo=ldo, mask=mask, drop_p=drop_p, cs_tab=cs_tab, idx=idx, v32=v32,
                g64=g64, mag=mag)


def _run_bwd(drn, c, M, N, dtype, three_d, colsum=None, colpart=None):
    grad = c["parts"].to(DEV)
    grad = grad[:, :M, :N] if three_d else grad[0, :M, :N]
    dpre = torch.full((M + 1, c["ldo"]), 7.0, dtype=dtype, device=DEV)
    ldT = (M + 7) // 8 * 8 + 8
    dpreT = torch.full((N + 1, ldT), 7.0, dtype=dtype, device=DEV)
    drn.bias_act_bwd(grad, M, N, saved=c["saved"].to(DEV), mask=None if c["mask"] is None else c["mask"].to(DEV),
                     drop_p=c["drop_p"], colscale=c["cs_tab"].to(DEV), dpre=dpre, dpreT=dpreT, colsum=colsum, colpart=colpart,
                     colidx=None if c["idx"] is None else c["idx"].to(DEV))
    return dpre, dpreT


def _check_dpre(c, dpre, dpreT, M, N, dtype):
    want = c["v32"].to(dtype)
    assert torch.equal(dpre.cpu()[:M, :N], want)
    assert torch.equal(dpreT.cpu()[:N, :M], want.t())
    assert _untouched(dpre.float(), _region(dpre.shape, slice(0, M), slice(0, N)), 7.0)
    assert _untouched(dpreT.float(), _region(dpreT.shape, slice(0, N), slice(0, M)), 7.0)


def _check_colsums(drn, c, colpart, nparts, M, N, S):
    """colsum_reduce with accumulate 0 (over a NaN-filled colsum) and 1 (over random previous values) against fp64"""
    assert _untouched(colpart, _region(colpart.shape, slice(0, nparts), slice(0, N)), NAN)  # rows past nparts untouched
    ref = c["g64"].sum(0)
    bnd = gamma(M + S + 1) * c["mag"].sum(0)
    out = torch.full((N + 3,), NAN, device=DEV)
    drn.colsum_reduce(colpart, nparts, N, out, accumulate=False)
    o = out.cpu()
    assert bool(torch.isnan(o[N:]).all())
    err = (o[:N].double() - ref).abs()
    assert bool((err <= bnd).all()), float((err - bnd).max())
    prev = torch.from_numpy(np.random.RandomState(N).standard_normal(N + 3).astype(np.float32) * 10)
    out = prev.clone().to(DEV)
    drn.colsum_reduce(colpart, nparts, N, out, accumulate=True)
    o = out.cpu()
    assert torch.equal(o[N:], prev[N:])
    err = (o[:N].double() - (prev[:N].double() + ref)).abs()
    assert bool((err <= gamma(M + S + 2) * (prev[:N].double().abs() + c["mag"].sum(0))).all())
    return o[:N], prev[:N]


TWO_STAGE = [(1, 103, torch.float32), (63, 103, torch.bfloat16), (64, 103, torch.float32), (65, 103, torch.bfloat16),
             (2000, 103, torch.float32), (4096 + 17, 103, torch.bfloat16), (65, 4096 + 3, torch.float32),
             (4096 + 17, 4096 + 3, torch.bfloat16), (1025, 1028, torch.bfloat16),  # N % 4 == 0, bf16: the vectorised kernel
             (2000, 1028, torch.bfloat16), (4096 + 17, 1028, torch.float32)]


@pytest.mark.parametrize("M,N,dtype", TWO_STAGE)
def test_colsum_two_stage(drn, M, N, dtype):
    """bias_act_bwd(colpart=...) then colsum_reduce, as flush_colsums runs them: nparts = ceil(M / 64) crosses the 16
    partials per trip of colsum_reduce_kernel; the one-pass colsum= call gives the same bits"""
    rs = np.random.RandomState(M * 7 + N)
    mode = "mask" if (M + N) % 2 else "drop"
    c = _bwd_case(rs, M, N, 1, mode, dtype, colidx=False)
    nparts = (M + 63) // 64
    colpart = torch.full((nparts + 2, N), NAN, device=DEV)
    dpre, dpreT = _run_bwd(drn, c, M, N, dtype, False, colpart=colpart)
    _check_dpre(c, dpre, dpreT, M, N, dtype)
    _check_colsums(drn, c, colpart, nparts, M, N, 1)
    one = torch.full((N,), NAN, device=DEV)
    _run_bwd(drn, c, M, N, dtype, False, colsum=one)
    two = torch.full((N,), NAN, device=DEV)
    drn.colsum_reduce(colpart, nparts, N, two)
    assert torch.equal(one.cpu(), two.cpu())


@pytest.mark.parametrize("M,N,S,dtype", [(65, 103, 1, torch.float32), (2000, 4096 + 3, 3, torch.bfloat16),
                                         (4096 + 17, 1028, 8, torch.bfloat16), (1, 103, 8, torch.float32),
                                         (1025, 1028, 3, torch.float32), (64, 1028, 1, torch.bfloat16)])
def test_bias_act_bwd_splits(drn, M, N, S, dtype):
    """drn_bias_act_bwd_splits: 3-D fp32 split-K grad_out (split stride != M * ld) summed on load, per-loss column scales
    through colidx (-1 = 0); dpre / dpreT bit-exact to the fp32 sum in split order, the column sums against fp64"""
    rs = np.random.RandomState(S * 1000 + M + N)
    c = _bwd_case(rs, M, N, S, "drop" if S % 2 else "mask", dtype, colidx=True)
    nparts = (M + 63) // 64
    colpart = torch.full((nparts + 2, N), NAN, device=DEV)
    dpre, dpreT = _run_bwd(drn, c, M, N, dtype, True, colpart=colpart)
    _check_dpre(c, dpre, dpreT, M, N, dtype)
    o, prev = _check_colsums(drn, c, colpart, nparts, M, N, S)
    off = c["idx"] < 0  # columns without an upstream loss: scale 0, the accumulated sum keeps its previous value
    assert bool(off.any()) and torch.equal(o[off], prev[off])


# ------------------------------------------------------------------------------------------- sum_small
@pytest.mark.parametrize("n", [1, 2, 7, 64, 1000])
def test_sum_small(drn, cabi, n):
    """drn_sum_small (the loss of a batch of several images): in-order fp32 sum times scale, within gamma_{n+1} sum|x|"""
    rs = np.random.RandomState(n)
    x = rs.standard_normal(n) * np.exp(rs.uniform(-6, 6, n))
    buf = torch.full((n + 5,), NAN, device=DEV)  # NaN past n: an over-read gives NaN
    buf[:n] = torch.from_numpy(x.astype(np.float32)).to(DEV)
    xs = buf[:n].cpu().double()
    for scale in (0.3, -2.75):
        out = torch.full((2,), NAN, device=DEV)
        cabi.call("drn_sum_small", cabi.ptr(buf), n, float(scale), cabi.ptr(out), cabi.stream())
        o = out.cpu()
        ref = float(xs.sum()) * _f32(scale)
        assert math.isnan(float(o[1]))
        assert abs(float(o[0]) - ref) <= gamma(n + 1) * float(xs.abs().sum()) * abs(_f32(scale))
        assert torch.equal(drn.sum_small(buf[:n], scale).cpu(), o[:1])


# ------------------------------------------------------------------------------------------- mean_softmax
def _msm_logits(rs, M, C, H, gap):
    """head windows of C columns, `gap` NaN columns between and around them, NaN in row M: rows of N(0, 3) logits, rows
    spread over +-1e4 (exp overflows unless the maximum is subtracted) and rows of equal logits"""
    col0s = [gap + h * (C + gap) for h in range(H)]
    ld = col0s[-1] + C + gap
    lg = torch.full((M + 1, ld), NAN)
    for h, c0 in enumerate(col0s):
        x = rs.standard_normal((M, C)) * 3
        spread = np.arange(M) % 3 == 1
        x[spread] = rs.uniform(-1e4, 1e4, (int(spread.sum()), C))
        x[np.arange(M) % 7 == 2] = 5.5 if h % 2 else -1e4
        lg[:M, c0: c0 + C] = torch.from_numpy(x.astype(np.float32))
    return lg, col0s, ld


@pytest.mark.parametrize("H", [1, 2, 4])
@pytest.mark.parametrize("C", [2, 21, 64, 65, 81, 256, 257, 1231])
def test_mean_softmax(drn, cabi, C, H):
    """drn_mean_softmax (inference / TTA): the wave kernel (C <= 64), the LDS kernel (C <= 256) and the in-row kernel
    (C > 256), with the wave kernel on and off, bg_first, ragged M; against the fp64 mean of softmaxes"""
    M = 131
    rs = np.random.RandomState(C * 10 + H)
    lg, col0s, ld = _msm_logits(rs, M, C, H, 3)
    x64 = torch.stack([lg[:M, c: c + C].double() for c in col0s])  # [H, M, C]
    p64 = torch.softmax(x64, -1).mean(0)
    rel = torch.stack([_softmax_rel_bound(x64[h], C) for h in range(H)]).max(0).values
    bnd = (2 * (rel + gamma(H + 1)))[:, None] * p64 + 2.0 ** -120  # x2: the second-order terms of the first-order bound
    lgd = lg.to(DEV)
    cd = torch.tensor(col0s, dtype=torch.int32, device=DEV)
    res = {}
    for wave in (1, 0):
        with drn.tuned({drn.TUNE_MSM_WAVE: wave}):
            for bg in (False, True):
                probs = torch.full((M + 1, C), NAN, device=DEV)
                cabi.call("drn_mean_softmax", cabi.ptr(lgd), ld, cabi.ptr(cd), H, C, cabi.ptr(probs), M, int(bg), cabi.stream())
                res[wave, bg] = probs.cpu()
    for (wave, bg), p in res.items():
        assert bool(torch.isnan(p[M]).all())
        ref, b = (torch.cat([p64[:, 1:], p64[:, :1]], 1), torch.cat([bnd[:, 1:], bnd[:, :1]], 1)) if bg else (p64, bnd)
        err = (p[:M].double() - ref).abs()
        assert bool((err <= b).all()), (wave, bg, float((err - b).max()))
    # both kernels sum in class order: the same bits with the wave kernel on or off
    assert torch.equal(res[1, False][:M], res[0, False][:M]) and torch.equal(res[1, True][:M], res[0, True][:M])
    assert torch.equal(res[1, True][:M, :-1], res[1, False][:M, 1:])
    assert torch.equal(drn.mean_softmax(lgd[:M], col0s, C).cpu(), res[1, False][:M])


# ------------------------------------------------------------------------------------------- softmax_ce
def _ce_call(cabi, lgd, ld, col0, C, lab, w, probs, dl, ld_d, loss, scratch, M, scale):
    cabi.call("drn_softmax_ce", cabi.ptr(lgd), ld, col0, C, cabi.ptr(lab), cabi.ptr(w), cabi.ptr(probs), cabi.ptr(dl), ld_d,
              cabi.ptr(loss), cabi.ptr(scratch), M, float(scale), cabi.stream())


def _ce_case(rs, M, C, col0, ld):
    lg = torch.full((M + 1, ld), NAN)
    x = rs.standard_normal((M, C)) * 3
    big = np.arange(M) % 4 == 1
    x[big] = rs.standard_normal((int(big.sum()), C)) * 1e4  # huge logits: loss terms of ~1e4
    labels = rs.randint(-1, C, M)
    labels[::17] = -1
    huge = np.arange(M) % 9 == 4
    x[huge] = rs.standard_normal((int(huge.sum()), C)) * 1e30  # exp of everything but the maximum is 0
    labels[huge] = x[huge].argmax(1)
    lg[:M, col0: col0 + C] = torch.from_numpy(x.astype(np.float32))
    w = rs.rand(M).astype(np.float32)
    w[::5] = 0
    return lg, torch.from_numpy(labels.astype(np.int32)), torch.from_numpy(w)


@pytest.mark.parametrize("C,M", [(6, 77), (21, 2000), (81, 1001), (128, 1001), (128, 16)])
def test_softmax_ce(drn, cabi, C, M):
    """drn_softmax_ce (the OICR refinement loss) against oicr_cls_loss on fp64 logits and its autograd gradient, with rows of
    huge logit magnitudes and C = 128, the kernel's limit"""
    rs = np.random.RandomState(C * 100 + M)
    col0, ld, ld_d, scale = 5, C + 9, C + 12, 0.61
    lg, labels, w = _ce_case(rs, M, C, col0, ld)
    x64 = lg[:M, col0: col0 + C].double().requires_grad_(True)
    L64 = O.oicr_cls_loss(x64, labels.long(), w.double())
    L64.backward()
    d64 = x64.grad * _f32(scale)
    p64 = torch.softmax(x64.detach(), -1)
    eps = _softmax_rel_bound(x64.detach(), C)
    # loss: per row |c^ - c| <= w (1.1 dS + 3 u (|log S| + |x_l - max| + |c|)), dS = (R + 5) u + gamma_C the sum's relative
    # error; rows summed within gamma_M; divided by the exact count V
    xd = x64.detach()
    mx = xd.max(-1).values
    lse = torch.logsumexp(xd - mx[:, None], -1)
    valid = labels >= 0
    wl = torch.where(valid, w.double(), torch.zeros((), dtype=torch.float64))
    xl = xd.gather(1, labels.long().clamp(min=0)[:, None])[:, 0]
    c = torch.where(valid, lse - (xl - mx), torch.zeros((), dtype=torch.float64))
    dS = (eps - (C + 16) * U) / 2 + 5 * U + gamma(C)
    E = (wl * (1.1 * dS + 3 * U * (lse.abs() + (xl - mx).abs() + c.abs()))).sum()
    V = float((wl > 1e-12).sum())
    lbound = 2 * ((E + gamma(M) * (wl * c).abs().sum()) / V + U * abs(float(L64.detach())))  # x2: second-order terms
    # dlogits: |f| (eps p + 4 u |p - onehot|) with f = w / V * scale; x2 as above
    f = (wl / V * _f32(scale))[:, None]
    onehot = F.one_hot(labels.long().clamp(min=0), C).double() * valid[:, None]
    dbound = 2 * (f.abs() * (eps[:, None] * p64 + 4 * U * (p64 - onehot).abs())) + 2.0 ** -120

    lgd = lg.to(DEV)
    nb = (M + 15) // 16
    probs = torch.full((M + 1, C), NAN, device=DEV)
    dl = torch.full((M + 1, ld_d), NAN, device=DEV)
    loss = torch.full((2,), NAN, device=DEV)
    scratch = torch.full((2 * nb + 4,), NAN, device=DEV)
    _ce_call(cabi, lgd, ld, col0, C, labels.to(DEV), w.to(DEV), probs, dl, ld_d, loss, scratch, M, scale)
    pc, dc, lc = probs.cpu(), dl.cpu(), loss.cpu()
    assert bool(torch.isnan(pc[M]).all()) and math.isnan(float(lc[1]))
    assert bool(((pc[:M].double() - p64).abs() <= 2 * eps[:, None] * p64 + 2.0 ** -120).all())
    assert abs(float(lc[0]) - float(L64)) <= lbound, (float(lc[0]), float(L64), float(lbound))
    win = _region(dl.shape, slice(0, M), slice(col0, col0 + C))
    assert _untouched(dl, win, NAN)
    err = (dc[:M, col0: col0 + C].double() - d64).abs()
    assert bool((err <= dbound).all()), float((err - dbound).max())
    # inference form (no labels): the same probabilities, nothing else written
    probs2 = torch.full((M + 1, C), NAN, device=DEV)
    _ce_call(cabi, lgd, ld, col0, C, None, None, probs2, None, 0, None, None, M, 1.0)
    assert torch.equal(probs2.cpu()[:M], pc[:M]) and bool(torch.isnan(probs2.cpu()[M]).all())


def test_softmax_ce_limits(drn, cabi):
    """C = 129 is refused and writes nothing.  A batch whose weights are all zero: oicr_cls_loss divides 0 by 0 - a NaN
    loss, NaN gradients in its labelled rows and zeros in the ignored ones.  The kernel returns the same NaN loss and
    writes NaN to every row of the head's dlogits window, the ignored ones included (0 / V with V = 0); the step is
    poisoned either way, so that choice is asserted here as it stands."""
    from drn_wsod_pytorch_amd._cabi import DrnError

    rs = np.random.RandomState(5)
    M, C, col0, ld = 40, 129, 1, 133
    lg = torch.from_numpy(rs.standard_normal((M, ld)).astype(np.float32)).to(DEV)
    labels = torch.from_numpy(rs.randint(0, C, M).astype(np.int32)).to(DEV)
    w = torch.ones(M, device=DEV)
    probs = torch.full((M, C), 7.0, device=DEV)
    dl = torch.full((M, ld), 7.0, device=DEV)
    loss = torch.full((1,), 7.0, device=DEV)
    scratch = torch.full((2 * ((M + 15) // 16),), 7.0, device=DEV)
    with pytest.raises(DrnError):
        _ce_call(cabi, lg, ld, col0, C, labels, w, probs, dl, ld, loss, scratch, M, 1.0)
    torch.cuda.synchronize()
    for b in (probs, dl, loss, scratch):
        assert bool((b.cpu() == 7.0).all())

    C, M = 21, 300
    lg, labels, w = _ce_case(rs, M, C, col0, C + 4)
    w = torch.zeros(M)
    x64 = lg[:M, col0: col0 + C].double().requires_grad_(True)
    L64 = O.oicr_cls_loss(x64, labels.long(), w.double())
    L64.backward()
    assert math.isnan(float(L64))
    assert bool(torch.isnan(x64.grad[labels >= 0]).all()) and bool((x64.grad[labels < 0] == 0).all())
    dl = torch.full((M, C + 6), 7.0, device=DEV)
    loss = torch.full((1,), 7.0, device=DEV)
    probs = torch.full((M, C), 7.0, device=DEV)
    scratch = torch.zeros((2 * ((M + 15) // 16),), device=DEV)
    _ce_call(cabi, lg.to(DEV), C + 4, col0, C, labels.to(DEV), w.to(DEV), probs, dl, C + 6, loss, scratch, M, 1.0)
    assert math.isnan(float(loss))
    dc = dl.cpu()
    assert bool(torch.isnan(dc[:, col0: col0 + C]).all())
    assert bool((dc[:, :col0] == 7.0).all()) and bool((dc[:, col0 + C:] == 7.0).all())
    p64 = torch.softmax(x64.detach(), -1)
    eps = _softmax_rel_bound(x64.detach(), C)
    assert bool(((probs.cpu().double() - p64).abs() <= 2 * eps[:, None] * p64 + 2.0 ** -120).all())


# ------------------------------------------------------------------------------------------- dropout masks
def _mask(drn, M, N, seed, count, p, dtype):
    """the keep mask and multipliers bias_act_fwd draws through the seed-counter path (zero partials, bias 1, ReLU)"""
    out = torch.zeros((M, N), dtype=dtype, device=DEV)
    dev = torch.full((1,), count, dtype=torch.int64, device=DEV)
    drn.bias_act_fwd(torch.zeros((1, M, N), device=DEV), M, N, torch.ones(N, device=DEV), True, None, seed=seed,
                     drop_p=p, out=out, seed_dev=dev)
    assert int(dev.item()) == count  # a dropout launch reads the counter; only the logits pass advances it
    return out


def _corr(a, b):
    a, b = a.double().flatten(), b.double().flatten()
    ma, mb = a.mean(), b.mean()
    return float(((a - ma) * (b - mb)).mean() / (a.var(unbiased=False) * b.var(unbiased=False)).sqrt())


@pytest.mark.parametrize("p", [0.5, 0.3])
def test_dropout_masks_as_the_step_draws_them(drn, p):
    """counter-based dropout (drn_drop_rule): keep-rate within 5 sigma of the binomial, per-row and per-column keep counts
    within a chi-square bound, fc6 / fc7 masks of one step and masks of consecutive steps uncorrelated, the scalar and the
    vectorised kernel and linear_act_fwd draw the same mask"""
    from drn_wsod_pytorch_amd.modeling import roi_heads as RH

    M, N = 2000, 4096
    seed, count = 0x5EED1234ABC, 3 * RH.DROP_COUNTER_STEP
    s6, s7 = RH.dropout_seeds(seed)
    q = 1.0 - math.ceil(_f32(p) * 2 ** 24) / 2 ** 24  # keep probability: 24-bit uniforms (p = 0.5: one hash bit)
    scale = float(torch.tensor(1.0) / (torch.tensor(1.0) - torch.tensor(p, dtype=torch.float32)))
    m6 = _mask(drn, M, N, s6, count, p, torch.bfloat16)
    m6f = _mask(drn, M, N, s6, count, p, torch.float32)  # act_kernel (per element) vs act_vec_kernel (four at a time)
    assert torch.equal(m6f.cpu() != 0, m6.cpu() != 0)
    assert bool(((m6f == 0) | (m6f == scale)).all())
    A = torch.zeros((M, 64), dtype=torch.bfloat16, device=DEV)
    W = torch.zeros((N, 64), dtype=torch.bfloat16, device=DEV)
    lin = torch.zeros((M, N), dtype=torch.bfloat16, device=DEV)
    dev = torch.full((1,), count, dtype=torch.int64, device=DEV)
    assert drn.linear_act_fwd(A, W, M, N, 64, torch.ones(N, device=DEV), True, None, s6, p, out=lin, seed_dev=dev)
    assert torch.equal(lin, m6)

    n = M * N
    k6 = (m6.cpu() != 0).double()
    assert abs(float(k6.sum()) - n * q) <= 5 * math.sqrt(n * q * (1 - q))
    for counts, trials, df in ((k6.sum(1), N, M), (k6.sum(0), M, N)):
        chi2 = float(((counts - trials * q) ** 2 / (trials * q * (1 - q))).sum())
        assert chi2 <= df + 5 * math.sqrt(2 * df), (chi2, df)
    others = {"fc7 of the step": _mask(drn, M, N, s7, count, p, torch.bfloat16),
              "fc6 of the next step": _mask(drn, M, N, s6, count + RH.DROP_COUNTER_STEP, p, torch.bfloat16),
              "counter + 1": _mask(drn, M, N, s6, count + 1, p, torch.bfloat16)}
    for what, m in others.items():
        k = (m.cpu() != 0).double()
        assert not torch.equal(k, k6), what
        assert abs(_corr(k, k6)) < 5 / math.sqrt(n), what
