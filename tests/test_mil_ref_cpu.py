"""The bounds of test_mil_ref_gpu.py held against the fp32 torch autograd oracle in place of the kernels: the same case
builders, fp64 references and bound functions (mil_ref_util.py).  Every bound must hold for plain fp32 arithmetic - they
are not tighter than the number format allows - and the conditions on the inputs that keep the cases away from the clamp
discontinuities hold for the committed seeds.  Each test prints error / bound per output (pytest -s)."""
import numpy as np
import pytest
import torch

import mil_ref_util as R


def test_clamp_constants():
    """the oracle's torch.clamp(min=1e-6, max=1.0 - 1e-6) on an fp32 tensor uses these fp32 values, as the kernel's
    1e-6f and 1.0f - 1e-6f do; 1 - hi is exact in fp32"""
    assert np.float32(1.0 - 1e-6) == np.float32(1) - np.float32(1e-6) == np.float32(R.HI)
    x = torch.tensor([0.0, 2.0])
    assert torch.equal(torch.clamp(x, min=1e-6, max=1.0 - 1e-6).double(), torch.tensor([R.LO, R.HI], dtype=torch.float64))
    assert float(np.float32(1) - np.float32(R.HI)) == 1.0 - R.HI


@pytest.mark.parametrize("case", R.WSDDN_CASES, ids=R.case_id)
def test_wsddn_bounds_hold_for_the_fp32_oracle(case):
    K, M_per, mean, scale, sat, _ = case
    cls, det, oh, sat_imgs = R.build_wsddn_case(K, M_per, sat)
    ref = R.wsddn_ref(cls, det, M_per, oh, mean, scale)
    R.wsddn_conditions(ref, M_per, sat_imgs)
    assert abs(float(ref["parts"].sum() - ref["loss"])) <= 1e-12 * abs(float(ref["loss"]))
    bnd = R.wsddn_bounds(ref, cls, det, M_per, oh, scale)
    o32 = R.wsddn_ref(cls, det, M_per, oh, mean, scale, dtype=torch.float32)
    ratios = R.wsddn_errors(o32, ref, bnd, M_per, sat_imgs)
    print("RATIO wsddn-fp32-oracle %s %s" % (R.case_id(case), " ".join("%s=%.3g" % kv for kv in sorted(ratios.items()))))
    r0 = 0
    for i, n in enumerate(M_per):  # det column 1 is constant: b = 1 / n
        if n >= 2 and K >= 4:
            assert bool((ref["b"][r0: r0 + n, 1] - 1.0 / n).abs().max() <= 1e-15)
        r0 += n


@pytest.mark.parametrize("K,M,mean", R.CSC_CASES)
def test_csc_bounds_hold_for_the_fp32_oracle(K, M, mean):
    cls, det, W, oh = R.build_csc_case(K, M)
    out = []
    for w in (W, None) if K >= 2 else (W,):
        ref = R.csc_ref(cls, det, w, oh, mean)
        R.csc_conditions(ref, w)
        bnd = R.csc_bounds(ref, cls, det, oh, mean)
        o32 = R.csc_ref(cls, det, w, oh, mean, dtype=torch.float32)
        out.append(("W" if w is not None else "ones", R.csc_errors(o32, ref, bnd)))
        if w is None:
            assert float(ref["neg"]) <= 1.1e-20 * K and float(o32["neg"]) <= 1.1e-20 * K
    for c in R.csc_seed_classes(K):
        ref = R.csc_ref(cls, det, None, oh, mean, seed_class=c)
        bnd = R.csc_bounds(ref, cls, det, oh, mean, seed_class=c)
        o32 = R.csc_ref(cls, det, None, oh, mean, seed_class=c, dtype=torch.float32)
        out.append(("seed%d" % c, R.csc_errors(o32, ref, bnd)))
    for name, r in out:
        print("RATIO csc-fp32-oracle K%d-M%d-%s %s %s" % (K, M, "mean" if mean else "sum", name,
                                                         " ".join("%s=%.3g" % kv for kv in sorted(r.items()))))


@pytest.mark.parametrize("K,M_per,nh,splits", R.FUSED_CASES)
def test_fused_case_inputs(K, M_per, nh, splits):
    """the logits drn_mil_oicr_losses forms (fp32 sum of the partials in split order, plus the bias) are within
    gamma_{splits+1} (sum|part| + |bias|) of the fp64 sum, and the WSDDN conditions hold on them"""
    c = R.build_fused_case(K, M_per, nh, splits)
    ow = c["owned"]
    err = (c["logits"].double() - c["exact"])[:, ow].abs()
    assert bool((err <= c["bound"][:, ow]).all())
    assert bool(torch.isnan(c["logits"][:, ~ow]).all())
    cls, det = c["logits"][:, c["c_cls"]: c["c_cls"] + K], c["logits"][:, c["c_det"]: c["c_det"] + K]
    ref = R.wsddn_ref(cls, det, M_per, c["oh"], True, 1.0)
    R.wsddn_conditions(ref, M_per, c["sat"])
    bnd = R.wsddn_bounds(ref, cls, det, M_per, c["oh"], 1.0)
    R.wsddn_errors(R.wsddn_ref(cls, det, M_per, c["oh"], True, 1.0, dtype=torch.float32), ref, bnd, M_per, c["sat"])
