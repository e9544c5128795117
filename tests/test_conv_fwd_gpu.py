"""Every forward conv kernel against float64 at its tile edges (cases, references and checks: conv_fwd_util.py; their own checks and
the planted faults they must see: test_conv_fwd_cpu.py).

conv_fwd_plan (csrc/conv.hip) picks one of eleven kernels.  The specialised bf16 ones are held bit-identical to the register-staged
tiled kernel elsewhere (test_conv_ring_kernels, test_pp8_conv_kernel, test_conv1x1_pp_kernel, test_conv3x3_c64_patch_kernel), at
every ring depth, schedule variant and real-size map; here each kernel - pinned through ops.tuned, and asserted with
ops.conv2d_plan before its result is trusted - runs the smallest shapes that still have a ragged row tile, a ragged column tile, an
image boundary inside a tile and a ring that is not full, in four epilogue forms (FrozenBN affine + ReLU, affine + shortcut,
affine + shortcut + ReLU, the VGG bias + ReLU), on two inputs:

  general input   every output element inside  4 eps32 sqrt(Cin k k) mag |scale| + 1e-6 + e_store(out dtype) |ref|  of the float64
                  conv * scale + bias (+ res * res_mult) -> ReLU of the stored operands; printed as RATIO <kind> <case> <value>;
  exact grid      operands on a coarse binary grid, so that fp32 accumulation in any order and the epilogue are exact and the only
                  rounding is the store: the output equals float64 -> float32 -> out dtype bit for bit (torch.equal on bf16 and
                  fp32, equal bytes on fp8), which also pins round-to-nearest-even at the store - the grid produces ties.

Mixed storage through conv2d_nhwc_q (bf16 operands -> fp32 output; an fp32 shortcut times 0.5 -> bf16 output; the fp8 recipe's
stem: bf16 operands -> fp8 e4m3fn output, on the grid alone) runs on one KS and one TILED_64 shape, and never on a bf16-only kernel.

Measured on an MI355X when these tests were written: the worst error / bound of the general-input check over all shapes and epilogue
forms of a kernel (1 is the bound; in bf16 the store's own half ulp is nearly all of it), and the result of the grid check:

    kernel         bf16 general  bf16 grid   fp32 general  fp32 grid
    PATCH_C64      0.9737        bit-exact   -             -
    PP256          0.9938        bit-exact   -             -
    PP8            0.9921        bit-exact   -             -          (3, 4 and 5 ring stages alike)
    PP8_WIDE       0.9921        bit-exact   -             -
    RING_64        0.9921        bit-exact   -             -
    RING_128       0.9921        bit-exact   -             -
    K2             0.9863        bit-exact   0.0305        bit-exact
    KS             0.9818        bit-exact   0.0147        bit-exact
    TILED_64       0.9917        bit-exact   0.1393        bit-exact
    TILED_128X64   0.9929        bit-exact   0.1238        bit-exact
    TILED_128      0.9948        bit-exact   0.1316        bit-exact

    mixed storage (bf16 operands)          KS general   TILED_64 general   grid
    fp32 output                            0.0026       0.0131             bit-exact
    fp32 shortcut x 0.5 -> bf16 output     0.9555       0.9867             bit-exact
    fp8 e4m3fn output                      -            -                  equal bytes
"""
import importlib

import pytest
import torch

import conv_fwd_util as V
from __graft_entry__ import load_package

pytestmark = pytest.mark.gpu
DEV = "cuda"


@pytest.fixture(scope="module")
def drn():
    assert torch.cuda.is_available(), "GPU tests need a GPU (run with -m gpu on the MI355X box)"
    pkg = load_package()
    pkg._cabi.lib()  # raises if the HIP library is missing: no fallback
    return importlib.import_module("drn_wsod_pytorch_amd.ops")


def _run(drn, case, form, kind):
    """the device's output as a CPU [N,Cout,Ho,Wo] tensor of the output dtype, from the kernel the case claims"""
    args = V.call_args(drn, case, form, kind, device=DEV)
    with drn.tuned(V.knob_dict(drn, case)):
        plan = drn.conv2d_plan(*args)
        assert V.KIND_NAMES.get(plan) == case.kind, (V.case_id(case), form, kind, plan)  # this run is the kernel the case is named after
        y = drn.conv2d_nhwc_q(*args)
        torch.cuda.synchronize()
    if case.out_dtype != case.dtype or case.res_dtype != case.dtype:
        assert case.kind not in V.BF16_ONLY_KINDS
    assert y.dtype == case.out_dtype
    if y.dtype == V.FP8:  # (moved as bytes)
        return V.nchw(y.view(torch.uint8).cpu().view(V.FP8))
    return V.nchw(y.cpu())


@pytest.mark.parametrize("cf", V.CASE_FORMS, ids=V.case_form_id)
def test_conv_forward_kernel(drn, cf):
    case, form = cf
    tag = "%s %s-%s-%s" % (case.kind, V.dname(case.dtype), case.tag, form)
    failures = []
    for kind in case.inputs:
        got = _run(drn, case, form, kind)
        ref, bound = V.reference(case, form, kind)
        assert got.shape == ref.shape
        if kind == "general":
            r = V.general_ratio(got.float(), ref, bound)
            print("RATIO %s %.4f" % (tag, r))
            if not r <= 1.0:
                failures.append(("general input: worst error / bound", r))
        else:
            bad = V.grid_mismatches(got.contiguous(), ref, case.out_dtype)
            print("GRID %s %s" % (tag, "bit-exact" if not bad else bad))
            if bad:
                failures.append(("exact grid: (index, device, expected)", bad))
    assert not failures, (tag, failures)
