"""drn_wsddn_fwd_bwd, the WSDDN stages of drn_mil_oicr_losses and drn_csc_loss against fp64 references at their block edges:
the second trip of the cross-block combine (images above 2048 rows at K <= 32, above 4096 at K > 32), both lane widths up
to K = 128, more than eight split-K partials, the clamp edges of the image score, ragged / one-row / empty images in one
batch, offset column windows, odd pitches and exactly the documented scratch size.

Case builders, references and the derivation of every bound are in mil_ref_util.py; test_mil_ref_cpu.py holds the same
bounds against the fp32 torch oracle.  The checks are element-wise (err <= bound everywhere).  Inputs are built on the CPU
from fixed seeds; output buffers are larger than what an op owns and pre-filled with NaN (7.0 for the refusals), input
buffers hold NaN wherever an op has no business reading, the scratch is NaN as well (a partial read before it is written
gives NaN).  Each test prints error / bound per output (pytest -s)."""
import math

import numpy as np
import pytest
import torch

import mil_ref_util as R
from __graft_entry__ import load_package

pytestmark = pytest.mark.gpu
DEV = "cuda"
NAN = float("nan")


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


def _nan_outside(buf, rows, cols):
    """every element of the 2-D buffer outside rows x cols (a list of column slices) is still NaN"""
    region = torch.zeros(buf.shape, dtype=torch.bool)
    for c in cols:
        region[rows, c] = True
    return bool(torch.isnan(buf[~region]).all())


def _show(tag, name, ratios):
    print("RATIO %s %s %s" % (tag, name, " ".join("%s=%.3g" % kv for kv in sorted(ratios.items()))))


# ------------------------------------------------------------------------------------------- drn_wsddn_fwd_bwd
def _layout(K):
    c_cls, c_det, ld = 3, 3 + K + 2, 2 * K + 11
    return c_cls, c_det, ld, ld + 3


def _scratch_floats(n_img, max_rows):
    return n_img * ((max_rows + 31) // 32) * 384  # include/drn_wsod.h


def _wsddn_buffers(cls, det, M_per, oh, fill=NAN, max_rows=None):
    M, K = cls.shape
    n_img = len(M_per)
    c_cls, c_det, ld, ld_d = _layout(K)
    lg = torch.full((M + 1, ld), NAN)  # NaN outside the two windows and in row M
    lg[:M, c_cls: c_cls + K], lg[:M, c_det: c_det + K] = cls, det
    ohb = torch.full((n_img + 1, K), NAN)
    ohb[:n_img] = oh
    off = torch.tensor([0] + list(np.cumsum(M_per)), dtype=torch.int32)
    f = lambda *shape: torch.full(shape, fill, device=DEV)
    max_rows = max(max(M_per), 1) if max_rows is None else max_rows
    return dict(lg=lg.to(DEV), oh=ohb.to(DEV), off=off.to(DEV), scores=f(M + 1, K), rowsm=f(M + 1, K), img=f(n_img + 1, K),
                parts=f(n_img + 2), dl=f(M + 1, ld_d), scratch=f(_scratch_floats(n_img, max_rows) + 64))


def _wsddn_call(cabi, b, K, n_img, max_rows, mean, scale, with_d=True):
    c_cls, c_det, ld, ld_d = _layout(K)
    cabi.call("drn_wsddn_fwd_bwd", cabi.ptr(b["lg"]), ld, c_cls, c_det, K, cabi.ptr(b["off"]), n_img, cabi.ptr(b["oh"]),
              cabi.ptr(b["scores"]), cabi.ptr(b["rowsm"]), cabi.ptr(b["img"]), cabi.ptr(b["parts"]),
              cabi.ptr(b["dl"]) if with_d else None, ld_d if with_d else 0, cabi.ptr(b["scratch"]), max_rows, int(mean),
              float(scale), cabi.stream())
    torch.cuda.synchronize()
    return {k: b[k].cpu() for k in ("scores", "rowsm", "img", "parts", "dl", "scratch")}


@pytest.mark.parametrize("case", R.WSDDN_CASES, ids=R.case_id)
def test_wsddn_fwd_bwd(drn, cabi, case):
    """every output of drn_wsddn_fwd_bwd within its derived bound of the fp64 reference, element by element; clamped image
    scores equal to the clamp constants bit for bit with an exactly zero gradient in that image's rows; an image without
    proposals gets img_scores = 1e-6, the BCE of that row and no gradient; nothing outside the owned regions is written,
    the scratch of the documented size suffices; a second run gives the same bits; dlogits = NULL gives the same forward
    outputs bit for bit and writes nothing else"""
    K, M_per, mean, scale, sat, extra = case
    M, n_img = sum(M_per), len(M_per)
    cls, det, oh, sat_imgs = R.build_wsddn_case(K, M_per, sat)
    ref = R.wsddn_ref(cls, det, M_per, oh, mean, scale)
    R.wsddn_conditions(ref, M_per, sat_imgs)
    bnd = R.wsddn_bounds(ref, cls, det, M_per, oh, scale)
    c_cls, c_det, ld, ld_d = _layout(K)
    max_rows = max(M_per) + extra
    runs = [_wsddn_call(cabi, _wsddn_buffers(cls, det, M_per, oh, max_rows=max_rows), K, n_img, max_rows, mean, scale, with_d)
            for with_d in (True, True, False)]
    o = runs[0]
    # nothing but the owned regions is written
    assert bool(torch.isnan(o["scores"][M]).all()) and bool(torch.isnan(o["rowsm"][M]).all())
    assert bool(torch.isnan(o["img"][n_img]).all()) and bool(torch.isnan(o["parts"][n_img:]).all())
    assert _nan_outside(o["dl"], slice(0, M), [slice(c_cls, c_cls + K), slice(c_det, c_det + K)])
    assert bool(torch.isnan(o["scratch"][_scratch_floats(n_img, max_rows):]).all())
    assert not bool(torch.isnan(o["dl"][:M, c_cls: c_cls + K]).any()) and not bool(torch.isnan(o["dl"][:M, c_det: c_det + K]).any())
    got = dict(a=o["rowsm"][:M], s=o["scores"][:M], img=o["img"][:n_img], parts=o["parts"][:n_img],
               dcls=o["dl"][:M, c_cls: c_cls + K], ddet=o["dl"][:M, c_det: c_det + K])
    _show("wsddn", R.case_id(case), R.wsddn_errors(got, ref, bnd, M_per, sat_imgs))
    r0 = 0
    for i, n in enumerate(M_per):
        if n == 0:  # predict_probs_img on an empty split
            assert bool((got["img"][i] == np.float32(R.LO)).all())
        if n >= 2 and K >= 4 and n & (n - 1) == 0:  # constant det column, n a power of two: b = 1 / n exactly
            assert torch.equal(got["s"][r0: r0 + n, 1], got["a"][r0: r0 + n, 1] * (1.0 / n))
        r0 += n
    # determinism; the forward outputs do not depend on dlogits
    for k in ("scores", "rowsm", "img", "parts", "dl"):
        assert torch.equal(o[k].view(torch.int32), runs[1][k].view(torch.int32)), k
    for k in ("scores", "rowsm", "img", "parts"):
        assert torch.equal(o[k].view(torch.int32), runs[2][k].view(torch.int32)), k
    assert bool(torch.isnan(runs[2]["dl"]).all())


def test_wsddn_refusals(drn, cabi):
    """K = 129, K = 0, n_img = 0 and max_rows = 0 are refused, and nothing is written"""
    K, M_per = 20, [40, 33]
    cls, det, oh, _ = R.build_wsddn_case(K, M_per)
    for k_arg, n_img, max_rows in ((129, 2, 40), (0, 2, 40), (K, 0, 40), (K, 2, 0)):
        b = _wsddn_buffers(cls, det, M_per, oh, fill=7.0, max_rows=40)
        with pytest.raises(cabi.DrnError):
            _wsddn_call(cabi, b, k_arg, n_img, max_rows, True, 1.0)
        torch.cuda.synchronize()
        for k in ("scores", "rowsm", "img", "parts", "dl", "scratch"):
            assert bool((b[k].cpu() == 7.0).all()), (k_arg, n_img, max_rows, k)


# ------------------------------------------------------------------------------------------- drn_mil_oicr_losses
def _gt_lists(oh, gmax=4):
    n_img = oh.shape[0]
    gcl = torch.zeros((n_img, gmax), dtype=torch.int32)
    gcn = torch.zeros((n_img,), dtype=torch.int32)
    for i in range(n_img):
        g = oh[i].nonzero().view(-1)
        gcl[i, : len(g)] = g.int()
        gcn[i] = len(g)
    return gcl.to(DEV), gcn.to(DEV)


def _boxes(M, seed, W=200, H=150):
    rs = np.random.RandomState(seed)
    x0, y0 = rs.rand(M) * (W - 30), rs.rand(M) * (H - 30)
    return torch.from_numpy(np.stack([x0, y0, x0 + 10 + rs.rand(M) * (W - x0 - 10), y0 + 10 + rs.rand(M) * (H - y0 - 10)],
                                     1).astype(np.float32))


@pytest.mark.parametrize("K,M_per,nh,splits", R.FUSED_CASES)
def test_mil_oicr_losses_logits_and_wsddn(drn, K, M_per, nh, splits):
    """the fused loss tail reading split-K partials (1, 8: the straight-line loader; 9, 16, 17: the any-number-of-splits
    one; NaN in every column no head owns and beyond NH): the logits it WRITES equal the fp32 sum in split order plus the
    bias bit for bit and lie within gamma_{splits+1} (sum|part| + |bias|) of the fp64 sum; its WSDDN outputs are within
    the bounds of test_wsddn_fwd_bwd of the fp64 reference on those logits"""
    c = R.build_fused_case(K, M_per, nh, splits)
    M, n_img, ldp, ow = sum(M_per), len(M_per), c["ldp"], c["owned"]
    c_cls, c_det = c["c_cls"], c["c_det"]
    pbuf = torch.full((splits, M + 1, ldp), NAN)
    pbuf[:, :M] = c["part"]
    pbuf = pbuf.to(DEV)
    gcl, gcn = _gt_lists(c["oh"])
    off = torch.tensor([0] + list(np.cumsum(M_per)), dtype=torch.int32, device=DEV)
    lg = torch.full((M + 1, ldp + 3), NAN, device=DEV)
    dl = torch.full((M + 1, ldp + 5), NAN, device=DEV)
    sc, img, parts, chain = drn.mil_oicr_losses(pbuf[:, :M], c["bias"].to(DEV), lg[:M], c_cls, c_det, K, off, n_img,
                                                c["oh"].to(DEV), c["col0s"], _boxes(M, 35).to(DEV), gcl, gcn, dlogits=dl[:M],
                                                mean_loss=True, loss_scale=0.61, max_rows=max(M_per))
    torch.cuda.synchronize()
    lgc, dlc = lg.cpu(), dl.cpu()
    assert bool(torch.isnan(lgc[M]).all()) and bool(torch.isnan(lgc[:, ldp:]).all()) and bool(torch.isnan(lgc[:M, :ldp][:, ~ow]).all())
    w = lgc[:M, :ldp][:, ow]
    err = (w.double() - c["exact"][:, ow]).abs()
    assert bool((err <= c["bound"][:, ow]).all()), R.ratio(err, c["bound"][:, ow])
    assert torch.equal(w, c["logits"][:, ow])
    cls, det = lgc[:M, c_cls: c_cls + K].clone(), lgc[:M, c_det: c_det + K].clone()
    ref = R.wsddn_ref(cls, det, M_per, c["oh"], True, 0.61)
    R.wsddn_conditions(ref, M_per, c["sat"])
    bnd = R.wsddn_bounds(ref, cls, det, M_per, c["oh"], 0.61)
    assert bool(torch.isnan(dlc[M]).all()) and bool(torch.isnan(dlc[:, ldp:]).all()) and bool(torch.isnan(dlc[:M, :ldp][:, ~ow]).all())
    got = dict(s=sc.cpu(), img=img.cpu(), parts=parts.cpu(), dcls=dlc[:M, c_cls: c_cls + K], ddet=dlc[:M, c_det: c_det + K])
    r = R.wsddn_errors(got, ref, bnd, M_per, c["sat"])
    r["logits"] = R.ratio(err, c["bound"][:, ow])
    _show("fused", "K%d-%s-s%d" % (K, "_".join(map(str, M_per)), splits), r)
    for k in range(nh):  # the refinement heads ran on the logits written by the same launch
        p = chain[k][1].cpu()
        p64 = torch.softmax(lgc[:M, c["col0s"][k]: c["col0s"][k] + K + 1].double(), -1)
        eps = R.softmax_rel_bound(lgc[:M, c["col0s"][k]: c["col0s"][k] + K + 1].double(), K + 1)
        assert bool(((p.double() - p64).abs() <= 2 * eps[:, None] * p64 + R.FLOOR_S).all()), k


# ------------------------------------------------------------------------------------------- drn_csc_loss
def _csc_call(cabi, b, K, M, W, oh, mode, cstar, mean, with_loss=True):
    c_cls, c_det, ld, ld_d = _layout(K)
    loss = torch.full((4,), NAN, device=DEV)
    dl = torch.full((M + 1, ld_d), NAN, device=DEV)
    cabi.call("drn_csc_loss", cabi.ptr(b["lg"]), ld, c_cls, c_det, K, M, cabi.ptr(b["scores"]), cabi.ptr(b["rowsm"]),
              cabi.ptr(W), cabi.ptr(oh), mode, cstar, int(mean), cabi.ptr(loss) if with_loss else None, cabi.ptr(dl), ld_d,
              cabi.stream())
    torch.cuda.synchronize()
    lc, dc = loss.cpu(), dl.cpu()
    assert _nan_outside(dc, slice(0, M), [slice(c_cls, c_cls + K), slice(c_det, c_det + K)])
    assert bool(torch.isnan(lc[2:]).all())
    return dict(pos=lc[0], neg=lc[1], dcls=dc[:M, c_cls: c_cls + K], ddet=dc[:M, c_det: c_det + K])


@pytest.mark.parametrize("K,M,mean", R.CSC_CASES)
def test_csc_loss(drn, cabi, K, M, mean):
    """drn_csc_loss on the scores / row softmax that drn_wsddn_fwd_bwd wrote, as the engine feeds it, against the fp64
    O.csc_losses and its autograd gradient end to end: signed W scaled so that sp, sn lie in (1e-3, 0.99); W = NULL (ones:
    sn = 0 is clamped to 1e-20 and passes no gradient; not for K = 1, where sp = 1 sits on the clamp edge and the
    reference gradient is discontinuous); the class-score seed at the first and last column and at both sides of the lane
    boundaries.  Rows M and beyond hold NaN in every input; M below, at and above one row pass of either lane width."""
    cls, det, W, oh = R.build_csc_case(K, M)
    b = _wsddn_buffers(cls, det, [M], oh.view(1, K))
    _wsddn_call(cabi, b, K, 1, M, True, 1.0, with_d=False)
    Wb = torch.full((M + 1, K), NAN)
    Wb[:M] = W
    Wd, ohd = Wb.to(DEV), torch.cat([oh, torch.full((3,), NAN)]).to(DEV)
    for name, w, wdev in (("W", W, Wd), ("ones", None, None)):
        if w is None and K == 1:
            continue
        ref = R.csc_ref(cls, det, w, oh, mean)
        R.csc_conditions(ref, w)
        got = _csc_call(cabi, b, K, M, wdev, ohd, 0, 0, mean)
        _show("csc", "K%d-M%d-%s-%s" % (K, M, "mean" if mean else "sum", name),
              R.csc_errors(got, ref, R.csc_bounds(ref, cls, det, oh, mean)))
        if w is None:
            assert float(got["neg"]) <= 1.1e-20 * K
        again = _csc_call(cabi, b, K, M, wdev, ohd, 0, 0, mean)
        for k in got:
            assert torch.equal(got[k].view(torch.int32), again[k].view(torch.int32)), k
    for c in R.csc_seed_classes(K):
        ref = R.csc_ref(cls, det, None, oh, mean, seed_class=c)
        got = _csc_call(cabi, b, K, M, None, None, 1, c, mean, with_loss=False)
        assert math.isnan(float(got.pop("pos"))) and math.isnan(float(got.pop("neg")))  # the seed mode writes no loss
        _show("csc", "K%d-M%d-seed%d" % (K, M, c), R.csc_errors(got, ref, R.csc_bounds(ref, cls, det, oh, mean, seed_class=c)))


def test_csc_refusals(drn, cabi):
    """K = 129, K = 0 and M = 0 are refused, and nothing is written"""
    K, M = 20, 40
    cls, det, W, oh = R.build_csc_case(K, M)
    b = _wsddn_buffers(cls, det, [M], oh.view(1, K))
    _wsddn_call(cabi, b, K, 1, M, True, 1.0, with_d=False)
    c_cls, c_det, ld, ld_d = _layout(K)
    ohd = oh.to(DEV)
    for k_arg, m_arg in ((129, M), (0, M), (K, 0)):
        loss = torch.full((2,), 7.0, device=DEV)
        dl = torch.full((M, ld_d), 7.0, device=DEV)
        with pytest.raises(cabi.DrnError):
            cabi.call("drn_csc_loss", cabi.ptr(b["lg"]), ld, c_cls, c_det, k_arg, m_arg, cabi.ptr(b["scores"]),
                      cabi.ptr(b["rowsm"]), None, cabi.ptr(ohd), 0, 0, 1, cabi.ptr(loss), cabi.ptr(dl), ld_d, cabi.stream())
        torch.cuda.synchronize()
        assert bool((loss.cpu() == 7.0).all()) and bool((dl.cpu() == 7.0).all())
