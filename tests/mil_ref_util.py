"""Case builders, fp64 references and derived error bounds of the MIL loss kernels (drn_wsddn_fwd_bwd, the WSDDN stages of
drn_mil_oicr_losses, drn_csc_loss), shared by test_mil_ref_cpu.py (the bounds against the fp32 torch oracle) and
test_mil_ref_gpu.py (the same bounds against the kernels); softmax_rel_bound is also the bound of test_heads_ref_gpu.py.

Arithmetic model: u = 2^-24; one fp32 operation is within u of exact, relative; an fp32 sum of n terms in ANY order (zero
addends are exact) is within gamma_n * sum|x_i|, gamma_n = n u / (1 - n u); expf / logf / log1pf are allowed 2 ulp = 4 u
(the device library documents 1 ulp for each).  Every bound below is first order in u and is DOUBLED at the end for the
second-order terms, plus an absolute floor for results below the normal range (an exp whose argument is under -87.3 is a
denormal or 0: that loses at most 2^-126 per factor).

WSDDN, per image of n rows, K classes; a = softmax over classes, b = softmax over the image's rows, s = a b:
  eps_a(r)  = softmax_rel_bound(cls, K)                                                     (C + 2 R + 16) u
  eps_b(c)  = softmax_rel_bound(det^T, n) + 5 u      the kernel forms the denominator as sum_blk bsum_blk * exp(bmax_blk - cmax):
              |x - bmax_blk| + |bmax_blk - cmax| = |x - cmax|, so the two subtractions round like the one of the plain form
              (the 2 R term); one more exp (4 u) and one more multiply (u); block, phase and cross-block sums together are one
              sum of n terms in some order, zeros included: gamma_n, the C = n of the bound
  eps_s     = eps_a + eps_b + u                                                             the product
  E_S(c)    = sum_r eps_s s + gamma_n S,  eps_S = E_S / S                                   S = sum_r s, all terms >= 0
  g_c       = (-(y / S) + (1 - y) / (1 - S)) * norm * scale inside the clamp range, else 0:
  eps_g     = eps_S * max(1, S / (1 - S)) + 6 u       1 - S (u, and the error of S amplified by S / (1 - S)), the division
              (u), norm = (1 / (n_img K)) / n_img (2 u), two multiplies (2 u)
  loss_i    = norm * sum_c t_c, t_c = -log S or -log(1 - S):  |dt_c| <= eps_S max(1, S / (1 - S)) + u + 4 u |t_c| (logf),
              clamped classes: u + 4 u |t_c| (the constants are exact, 1 - hi is exact); lane sum gamma_K sum|t_c|; norm and its
              multiply 3 u
  gradients, with G[r, c] = d loss / d s[r, c] (= g_c here) of relative error eps_G and gs = G s:
    d_cls[r, c] = gs_c - a_c * dot,  dot = sum_k gs_k:
        (eps_G + eps_s + 2 u) |gs_c| + a_c (sum_k (eps_G + eps_s + eps_a + 2 u) |gs_k| + (gamma_K + u) sum_k |gs_k|)
    d_det[r, c] = gs - b * T_c, T_c = sum_r gs  (the WSDDN kernel's g_c (s - b S_c) is the same expression with T = g S):
        (eps_G + eps_s + 2 u) |gs| + b (sum_r (eps_G + eps_s + u) |gs| + gamma_n sum_r |gs| + (eps_b + 2 u) sum_r |gs|)
  The bound multiplies eps by the sum of the ABSOLUTE values of the terms, so a cancellation cannot hide an error.

CSC (one image, drn_csc_loss): sp = sum_r s max(W, 0), sn = sum_r s max(-W, 0), clamp [1e-20, 1]:
  E_sp      = sum_r (eps_s + u) s w + gamma_n sp
  loss_pos  : t_c = -log sp or -log1p(-sp): eps_sp max(1, sp / (1 - sp)) + u + 4 u |t_c|; gamma_K; norm = 1 / K and its multiply 2 u
  gp        = (sp - y) / max((1 - sp) sp, 1e-12) * norm: sp - y and 1 - sp each carry E_sp / (1 - sp), the product eps_sp:
  eps_gp    = eps_sp (2 + 2 sp / (1 - sp)) + 6 u;  G = gp max(W, 0) + gn max(-W, 0) has one non-zero term: eps_G = eps_gp|gn + u
"""
import numpy as np
import torch
import torch.nn.functional as F

import golden_util as G

O = G.O
U = 2.0 ** -24
NAN = float("nan")
LO = float(np.float32(1e-6))  # the clamp constants of the image score: the fp32 values, widened
HI = float(np.float32(1) - np.float32(1e-6))
FLOOR_S = 2.0 ** -120  # absolute floors: scores / probabilities, and gradients (|G| <= 1e4 times a score)
FLOOR_G = 2.0 ** -100


def gamma(n):
    return n * U / (1 - n * U)


def f32(x):
    return float(np.float32(x))


def softmax_rel_bound(x64, C):
    """relative error bound of an fp32 softmax row computed as exp(x - max) / sum, per row: the subtraction's rounding
    scaled by |x - max| (R, over the entries whose exp is a normal number; the others are below 2^-126 and enter only the
    absolute 2^-120 of the callers), exp <= 2 ulp, the sum gamma_C, the division; first order: (C + 2 R + 16) u"""
    mx = x64.max(-1, keepdim=True).values
    d = (x64 - mx).abs()
    R = torch.where(d <= 88, d, torch.zeros(())).max(-1).values
    return (C + 2 * R + 16) * U


def ratio(err, bound):
    """largest error / bound of one output (what the summary reports; nothing is tuned to it)"""
    if err.numel() == 0:
        return 0.0
    return float((err / bound).max())


# --------------------------------------------------------------------------------------------------- WSDDN cases
# K, rows per image, mean_loss, loss_scale, saturated image (index, label "on" the saturated class / "off" = on a vanished
# one) or None, extra max_rows (grid blocks past the largest image)
WSDDN_CASES = [
    (1, [5], True, 1.0, None, 0),
    (2, [40, 1], False, 0.5, None, 0),
    (20, [2049, 31, 33], True, 0.61, None, 0),
    (20, [2049, 31, 33], False, 1.0, (1, "on"), 100),
    (32, [2080, 32], True, 0.5, (1, "off"), 0),
    (33, [4097, 5], True, 1.0, None, 0),
    (33, [4097, 5], False, 0.5, (1, "on"), 0),
    (64, [100], False, 0.61, None, 0),
    (65, [129, 1], True, 0.5, None, 0),
    (127, [64], True, 0.61, None, 0),
    (128, [4130, 64], True, 1.0, None, 0),
    (128, [4130, 64], False, 0.61, (1, "off"), 0),
    (20, [40, 0, 33], True, 0.61, None, 0),  # an image without proposals
    (65, [0, 40, 33], False, 1.0, (2, "on"), 0),
]


def case_id(c):
    K, M_per, mean, scale, sat, extra = c
    return "K%d-%s-%s-%g-%s-%d" % (K, "_".join(map(str, M_per)), "mean" if mean else "sum", scale,
                                  "sat%d%s" % sat if sat else "nosat", extra)


def case_seed(K, M_per):
    return 100003 * K + 17 * sum(M_per) + len(M_per)


def build_wsddn_case(K, M_per, sat=None, seed=None):
    """fp32 cls / det logits [M, K], labels [n_img, K] and the set of saturated images.  N(0, 1.5^2) logits; in every
    unsaturated image each row 1 mod 4 has cls logits of scale 1e4 (a one-hot row softmax; exp overflows unless the maximum
    is subtracted); up to three det columns have one row 60 above the rest (a one-hot column softmax; that row's cls logit
    is raised by 2 where K >= 8 so that S = a[r, c] stays above 1e-4), det column 1 is constant (b = 1 / n); the cls logits
    of an image of fewer than 8 rows are N(0, 0.5^2).  The saturated image has +30 on cls column c0 in every row: S[c0] -> 1
    (upper clamp), every other class below 1e-6 (lower clamp).  K = 1: S = 1, saturated by itself."""
    rs = np.random.RandomState(case_seed(K, M_per) if seed is None else seed)
    M, n_img = sum(M_per), len(M_per)
    cls = rs.standard_normal((M, K)) * 1.5
    det = rs.standard_normal((M, K)) * 1.5
    oh = np.zeros((n_img, K), np.float32)
    sat_imgs = set(i for i in range(n_img) if K == 1 and M_per[i] > 0)
    hot_cols = sorted({0, K - 1} | ({K // 2} if K >= 8 else set()))
    r0 = 0
    for i, n in enumerate(M_per):
        is_sat = sat is not None and sat[0] == i
        if n < 8:
            cls[r0: r0 + n] /= 3.0  # a tiny image: S[c] is close to one row's a[r, c], which must stay above 1e-4 for every c
        if n and not is_sat:
            big = r0 + np.nonzero(np.arange(n) % 4 == 1)[0]
            cls[big] = rs.standard_normal((len(big), K)) * 1e4
        if n >= 2:
            for j, c in enumerate(hot_cols):
                r = r0 + max(((n - 1) // 4) * 4 - 4 * j, 0)  # rows 0 mod 4 of the last blocks: never a 1e4 row
                det[r, c] = det[r0: r0 + n, c].max() + 60.0
                cls[r, c] += 2.0 if K >= 8 else 0.0
            if K >= 4:
                det[r0: r0 + n, 1] = 0.75
        if is_sat:
            assert n > 0
            c0 = min(2, K - 1)
            cls[r0: r0 + n, c0] += 30.0
            oh[i, c0 if sat[1] == "on" else (c0 + 1) % K] = 1
            sat_imgs.add(i)
        else:
            oh[i, (3 * i + 1) % K] = 1
            oh[i, (7 * i + 2) % K] = 1
        r0 += n
    return (torch.from_numpy(cls.astype(np.float32)), torch.from_numpy(det.astype(np.float32)), torch.from_numpy(oh),
            sat_imgs)


def wsddn_ref(cls, det, M_per, oh, mean_loss, loss_scale, dtype=torch.float64):
    """predict_probs_img + binary_cross_entropy_loss on softmax(cls, 1) * softmax(det, 0) per image, in `dtype` (fp64: the
    reference; fp32: the torch oracle the CPU test holds the bounds against), the gradient from autograd.  The clamp is to
    the fp32 constants; the loss is unscaled (as loss_part), the gradient is that of loss * fp32(loss_scale)."""
    n_img, K = oh.shape
    xc = cls.to(dtype).clone().requires_grad_(True)
    xd = det.to(dtype).clone().requires_grad_(True)
    a = F.softmax(xc, 1)
    b = torch.cat([F.softmax(d, 0) for d in xd.split(M_per)], 0)
    s = a * b
    S = torch.stack([x.sum(0) for x in s.split(M_per)])
    img = torch.clamp(S, min=LO, max=HI)
    y = oh.to(dtype)
    loss = F.binary_cross_entropy(img, y, reduction="mean" if mean_loss else "sum") / n_img
    (loss * f32(loss_scale)).backward()
    norm = (1.0 / (n_img * K) if mean_loss else 1.0) / n_img
    terms = F.binary_cross_entropy(img.detach(), y, reduction="none")
    return dict(a=a.detach(), b=b.detach(), s=s.detach(), S=S.detach(), img=img.detach(), loss=loss.detach(),
                terms=terms, parts=terms.sum(1) * norm, norm=norm, dcls=xc.grad, ddet=xd.grad)


def wsddn_conditions(ref, M_per, sat_imgs):
    """the conditions on the inputs, asserted on the fp64 reference by the CPU and the GPU test: the gradient is
    discontinuous at the clamp thresholds, so every S lies >= 1e-3 relative away from both (measured from 1e-6 and from
    1 - hi); S in [1e-4, 0.99] outside the saturated images (1 / (1 - S) <= 100); every class of a saturated image is
    outside the clamp range; an image without proposals has S = 0."""
    S = ref["S"]
    assert bool(((S - LO).abs() >= 1e-3 * LO).all()) and bool(((S - HI).abs() >= 1e-3 * (1 - HI)).all())
    for i, n in enumerate(M_per):
        if n == 0:
            assert bool((S[i] == 0).all())
        elif i in sat_imgs:
            assert bool(((S[i] < LO) | (S[i] > HI)).all()), (i, float(S[i].min()), float(S[i].max()))
        else:
            assert bool(((S[i] >= 1e-4) & (S[i] <= 0.99)).all()), (i, float(S[i].min()), float(S[i].max()))


def score_eps(cls64, det64, M_per):
    """eps_a [M], eps_b [M, K] (per image and column, spread over the image's rows), eps_s [M, K]"""
    K = cls64.shape[1]
    eps_a = softmax_rel_bound(cls64, K)
    eb = []
    for d, n in zip(det64.split(M_per), M_per):
        if n:
            eb.append((softmax_rel_bound(d.t(), n) + 5 * U)[None, :].expand(n, K))
    eps_b = torch.cat(eb, 0) if eb else torch.zeros((0, K), dtype=torch.float64)
    return eps_a, eps_b, eps_a[:, None] + eps_b + U


def grad_bounds(Gm, eps_G, ref, eps_a, eps_b, eps_s, M_per):
    """bounds of d_cls and d_det [M, K] for the objective with d / d s[r, c] = Gm[r, c] (relative error eps_G)"""
    K = Gm.shape[1]
    s, a, b = ref["s"], ref["a"], ref["b"]
    gs = Gm.abs() * s
    t1 = (eps_G + eps_s + 2 * U) * gs
    dot_err = ((eps_G + eps_s + eps_a[:, None] + 2 * U) * gs).sum(1, keepdim=True) + (gamma(K) + U) * gs.sum(1, keepdim=True)
    bcls = t1 + a * dot_err
    bdet, r0 = [], 0
    for n in M_per:
        sl = slice(r0, r0 + n)
        Tabs = gs[sl].sum(0)
        E_T = ((eps_G[sl] + eps_s[sl] + U) * gs[sl]).sum(0) + gamma(n) * Tabs
        bdet.append(t1[sl] + b[sl] * (E_T + (eps_b[sl] + 2 * U) * Tabs))
        r0 += n
    return 2 * bcls + FLOOR_G, 2 * torch.cat(bdet, 0) + FLOOR_G


def wsddn_bounds(ref, cls, det, M_per, oh, loss_scale):
    """element-wise bounds of every output of drn_wsddn_fwd_bwd: rowsm, scores [M, K], img_scores [n_img, K], loss_part
    [n_img], d_cls, d_det [M, K]"""
    n_img, K = oh.shape
    cls64, det64, y = cls.double(), det.double(), oh.double()
    eps_a, eps_b, eps_s = score_eps(cls64, det64, M_per)
    s, S, norm = ref["s"], ref["S"], ref["norm"]
    E_S = torch.stack([(e * x).sum(0) for e, x in zip(eps_s.split(M_per), s.split(M_per))]) \
        + torch.tensor([gamma(n) for n in M_per], dtype=torch.float64)[:, None] * S
    inside = (S >= LO) & (S <= HI)
    zero = torch.zeros((), dtype=torch.float64)
    eps_S = torch.where(inside, E_S / S.clamp(min=1e-300), zero)
    amp = torch.where(inside, (S / (1 - S)).clamp(min=1.0), zero)
    t = ref["terms"]
    e_c = eps_S * amp + U + 4 * U * t.abs()
    b_parts = 2 * (norm * (e_c.sum(1) + gamma(K) * t.abs().sum(1)) + 3 * U * ref["parts"].abs())
    eps_g = torch.where(inside, eps_S * amp + 6 * U, zero)
    g = torch.where(inside, (-(y / S.clamp(min=1e-300)) + (1 - y) / (1 - S)) * norm * f32(loss_scale), zero)
    rows = torch.repeat_interleave(torch.arange(n_img), torch.tensor(M_per))
    bcls, bdet = grad_bounds(g[rows], eps_g[rows], ref, eps_a, eps_b, eps_s, M_per)
    return dict(a=2 * eps_a[:, None] * ref["a"] + FLOOR_S, s=2 * eps_s * s + FLOOR_S,
                img=torch.where(inside, 2 * E_S, zero), parts=b_parts,
                loss=b_parts.sum() + gamma(n_img) * ref["parts"].abs().sum(), dcls=bcls, ddet=bdet, g=g)


def wsddn_errors(got, ref, bnd, M_per, sat_imgs):
    """compare one result set {a, s, img, parts, dcls, ddet} (fp32 tensors of the owned regions) with the reference:
    asserts every element-wise bound, the clamp constants bit for bit and the exactly-zero gradient where the clamp is
    active, returns error / bound per output"""
    out = {}
    for k in ("a", "s", "parts", "dcls", "ddet"):
        if k not in got:
            continue
        err = (got[k].double() - ref[k]).abs()
        assert bool((err <= bnd[k]).all()), (k, ratio(err, bnd[k]))
        out[k] = ratio(err, bnd[k])
    S = ref["S"]
    inside = (S >= LO) & (S <= HI)
    img = got["img"]
    assert bool((img[S < LO] == np.float32(LO)).all()) and bool((img[S > HI] == np.float32(HI)).all())
    err = (img.double() - ref["img"]).abs()
    assert bool((err <= bnd["img"]).all()), ("img", float((err - bnd["img"]).max()))
    out["img"] = ratio(err[inside], bnd["img"][inside]) if bool(inside.any()) else 0.0
    lerr = abs(float(got["parts"].double().sum()) - float(ref["loss"]))
    assert lerr <= float(bnd["loss"]), (lerr, float(bnd["loss"]))
    if "dcls" in got:
        r0 = 0
        for i, n in enumerate(M_per):
            if i in sat_imgs:  # the clamp passes no gradient: exact zeros in both windows
                assert bool((got["dcls"][r0: r0 + n] == 0).all()) and bool((got["ddet"][r0: r0 + n] == 0).all()), i
            elif n:
                assert float(got["dcls"][r0: r0 + n].abs().max()) > 0
                assert n == 1 or float(got["ddet"][r0: r0 + n].abs().max()) > 0  # one row: b = 1, no det gradient
            r0 += n
    return out


# --------------------------------------------------------------------------------------------------- CSC cases
# K, M, mean_loss: every M with both lane widths (K <= 32: 32 rows per pass, K > 32: 16)
CSC_CASES = [(1, 17, True), (4, 1, False), (4, 31, True), (31, 33, False), (32, 2049, True), (32, 32, False),
             (32, 15, True), (31, 16, False), (33, 1, True), (33, 15, False), (64, 16, True), (64, 17, False),
             (65, 31, True), (65, 32, False), (128, 33, True), (128, 2049, False)]


def csc_seed_classes(K):
    return sorted({c for c in (0, K - 1, 31, 32, 64) if c < K})


def build_csc_case(K, M):
    """one image of the WSDDN builder and signed weights W [M, K]: uniform signs and magnitudes, each sign's share of every
    column rescaled so that sp = sum_r s max(W, 0) and sn = sum_r s max(-W, 0) land on targets drawn from U(0.05, 0.9)"""
    cls, det, _, _ = build_wsddn_case(K, [M], None, seed=7919 * K + M)
    rs = np.random.RandomState(31 * K + M)
    s = (F.softmax(cls.double(), 1) * F.softmax(det.double(), 0)).numpy()
    W = rs.uniform(-1, 1, (M, K))
    for w, sign in ((np.maximum(W, 0), 1.0), (np.maximum(-W, 0), -1.0)):
        tot = (s * w).sum(0)
        tgt = rs.uniform(0.05, 0.9, K)
        W = np.where(w > 0, sign * w * (tgt / np.where(tot > 0, tot, 1.0))[None, :], W)
    oh = np.zeros(K, np.float32)
    oh[rs.permutation(K)[: max(1, K // 4)]] = 1
    return cls, det, torch.from_numpy(W.astype(np.float32)), torch.from_numpy(oh)


def csc_ref(cls, det, W, oh, mean_loss, seed_class=None, dtype=torch.float64):
    """CSCOutputs.csc_loss (O.csc_losses) on the WSDDN scores of one image in `dtype`, autograd for the gradient of
    loss_pos + loss_neg; seed_class: d (sum_r s[r, c]) / d logits instead.  W None = ones."""
    K = cls.shape[1]
    xc = cls.to(dtype).clone().requires_grad_(True)
    xd = det.to(dtype).clone().requires_grad_(True)
    a, b = F.softmax(xc, 1), F.softmax(xd, 0)
    s = a * b
    Wd = torch.ones_like(s) if W is None else W.to(dtype)
    wp, wn = Wd.clamp(min=0), (-Wd).clamp(min=0)
    ref = dict(a=a.detach(), b=b.detach(), s=s.detach(), wp=wp, wn=wn)
    if seed_class is not None:
        go = torch.zeros_like(s)
        go[:, seed_class] = 1
        ref["dcls"], ref["ddet"] = torch.autograd.grad(s, (xc, xd), grad_outputs=go)
        return ref
    L = O.csc_losses(s, wp, wn, oh.to(dtype).view(1, K), torch.zeros((1, K), dtype=dtype), mean_loss)
    (L["loss_cls_pos"] + L["loss_cls_neg"]).backward()
    ref.update(pos=L["loss_cls_pos"].detach(), neg=L["loss_cls_neg"].detach(), dcls=xc.grad, ddet=xd.grad,
               sp=(s.detach() * wp).sum(0), sn=(s.detach() * wn).sum(0))
    return ref


def csc_conditions(ref, W):
    """sp and sn inside (1e-3, 0.99) by construction; a column without a weight of one sign has an exact 0 there (every
    sn with W = None): clamped to 1e-20, no gradient.  With W = None sp is the image score: [1e-4, 0.99] as for WSDDN."""
    lo = 1e-3 if W is not None else 1e-4
    for x, w in ((ref["sp"], ref["wp"]), (ref["sn"], ref["wn"])):
        has = (w > 0).any(0)
        assert bool(((x > lo) & (x < 0.99))[has].all()), (float(x[has].min()), float(x[has].max()))
        assert bool((x[~has] == 0).all())


def csc_bounds(ref, cls, det, oh, mean_loss, seed_class=None):
    M, K = cls.shape
    eps_a, eps_b, eps_s = score_eps(cls.double(), det.double(), [M])
    s = ref["s"]
    zero = torch.zeros((), dtype=torch.float64)
    if seed_class is not None:
        Gm = torch.zeros_like(s)
        Gm[:, seed_class] = 1
        bcls, bdet = grad_bounds(Gm, torch.zeros_like(s), ref, eps_a, eps_b, eps_s, [M])
        return dict(dcls=bcls, ddet=bdet)
    y = oh.double()
    norm = 1.0 / K if mean_loss else 1.0
    out, gcol, ecol = {}, [], []
    for name, x, w, lab in (("pos", ref["sp"], ref["wp"], y), ("neg", ref["sn"], ref["wn"], torch.zeros_like(y))):
        live = x > 0
        E = ((eps_s + U) * s * w).sum(0) + gamma(M) * x
        eps_x = torch.where(live, E / x.clamp(min=1e-300), zero)
        xc = x.clamp(min=1e-20, max=1.0)
        amp = xc / (1 - xc)
        t = -(lab * torch.log(xc).clamp(min=-100) + (1 - lab) * torch.log1p(-xc).clamp(min=-100))
        e_c = eps_x * amp.clamp(min=1.0) + U + 4 * U * t.abs()
        out[name] = 2 * (norm * (e_c.sum() + gamma(K) * t.abs().sum()) + 2 * U * abs(float(ref[name]))) + 1e-30
        gcol.append(torch.where(live, (xc - lab) / ((1 - xc) * xc).clamp(min=1e-12) * norm, zero))
        ecol.append(torch.where(live, eps_x * (2 + 2 * amp) + 6 * U, zero))
    wp, wn = ref["wp"], ref["wn"]
    Gm = gcol[0][None, :] * wp + gcol[1][None, :] * wn
    eps_G = torch.where(wp > 0, ecol[0][None, :], ecol[1][None, :]) + U
    out["dcls"], out["ddet"] = grad_bounds(Gm, eps_G.expand_as(s), ref, eps_a, eps_b, eps_s, [M])
    return out


def csc_errors(got, ref, bnd):
    out = {}
    for k in ("pos", "neg", "dcls", "ddet"):
        if k not in got:
            continue
        err = (got[k].double() - ref[k]).abs()
        assert bool((err <= bnd[k]).all()), (k, ratio(err, bnd[k] + 0 * err))
        out[k] = ratio(err, bnd[k] + 0 * err)
    return out


# --------------------------------------------------------------------------------------------------- split-K partials
# K, rows per image, refinement heads, splits: the straight-line loader (<= 8) and the any-number-of-splits one
FUSED_CASES = [(6, [90, 77], 2, 1), (20, [100, 33], 1, 8), (80, [300], 2, 9), (20, [2049, 31], 3, 16), (33, [4097, 5], 2, 17)]


def build_fused_case(K, M_per, nh, splits):
    """predictor split-K partials [splits, M, ldp], bias [NH] and the column layout of drn_mil_oicr_losses: the cls window
    at column 1, det at K + 2, head k at 2K + 3 + k (K + 2), one unowned column in front of each (NaN in the bias and in every
    partial, as in the padding beyond NH).  The partials sum to the logits of the WSDDN builder (the last one takes the
    remainder), so the conditions on S hold; `logits` is the fp32 sum in split order plus the bias - the kernel's own
    IEEE additions, so the written logits must equal it bit for bit."""
    rs = np.random.RandomState(splits * 1009 + K)
    M = sum(M_per)
    cls, det, oh, sat = build_wsddn_case(K, M_per, None)
    c_cls, c_det = 1, K + 2
    col0s = [2 * K + 3 + k * (K + 2) for k in range(nh)]
    NH = col0s[-1] + K + 1
    ldp = (NH + 7) // 8 * 8 + 8
    owned = torch.zeros(ldp, dtype=torch.bool)
    owned[c_cls: c_cls + K] = owned[c_det: c_det + K] = True
    target = torch.zeros((M, ldp), dtype=torch.float64)
    target[:, c_cls: c_cls + K], target[:, c_det: c_det + K] = cls.double(), det.double()
    for c0 in col0s:
        owned[c0: c0 + K + 1] = True
        target[:, c0: c0 + K + 1] = torch.from_numpy(rs.standard_normal((M, K + 1)) * 3)
    bias = torch.from_numpy(rs.standard_normal(ldp).astype(np.float32))
    part = torch.from_numpy(rs.standard_normal((splits, M, ldp)).astype(np.float32))
    part[-1] = (target - bias.double() - part[:-1].double().sum(0)).float()
    v = torch.zeros((M, ldp))
    for q in range(splits):
        v = v + part[q]
    logits = v + bias
    logits[:, ~owned] = NAN  # never written: the sentinel of the logits buffer stays
    part[:, :, ~owned] = NAN
    bias[~owned] = NAN
    p64 = part.double()
    bound = gamma(splits + 1) * (p64.abs().sum(0) + bias.double().abs())
    return dict(part=part, bias=bias[:NH].clone(), logits=logits, exact=p64.sum(0) + bias.double(), bound=bound, owned=owned,
                c_cls=c_cls, c_det=c_det, col0s=col0s, NH=NH, ldp=ldp, oh=oh, sat=sat)
