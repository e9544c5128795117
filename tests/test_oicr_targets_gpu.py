"""drn_oicr_targets (stand-alone, per head inside drn_oicr_refine_chain, launch D of drn_mil_oicr_losses) against the numpy
reference of oicr_targets_util.py at the kernel's block edges: more than four classes (later and ragged mining trips),
rows past 2048 (second mining trip, third labelling loop), index ties at every tie site, the in-kernel zero-delta decode,
box_cols = 4K with differing class copies, two and three Matcher thresholds with IoUs exactly on them, no ground truth, and
images without proposals in every position.  Everything is torch.equal: integers and bit-exact floats, no tolerance.

Inputs are one row longer than M and that spare row holds values that would win / show if read (score 9, box 77777);
outputs are three rows (one image) longer than what the op owns and pre-filled with -77: every row of a non-empty image
must be overwritten, nothing else may be.  test_oicr_targets_cpu.py pins the reference to the oracle.

Case ids per code path (test_oicr_targets_cpu.py::test_every_code_path_is_reached prints the full lists, pytest -s):
  mining trips g0 >= 4       G5-* .. G17-*, K80-G80, K130-G128, batch-*, win-4097, ties-*, 4K-K20
  ragged last trip           G5-*, G7-*, G9-*, G17-*, batch-*, win-4097, ties-*, 4K-K5, 4K-K20
  mined row >= 2048          rows-2049 .. rows-5000, batch-37-2049-5, batch-4097-1-2048, win-4097, ties-*, K80-G80, 4K-K20
  third labelling loop       the same, and empty-last-decode
  tie inside a thread        ties-5000-props, ties-4100-decode (va / vb: rows 7 | 1031; two trips: 7 | 2055, 1500 | 2524)
  tie in the wave shuffle    rows-2 .. rows-65 (constant column), ties-* (130 | 131, 1030 | 2050, 3000 | 3001)
  tie in the LDS combine     rows-65, ties-* (400 | 1034, 63 | 64, the constant and the all-zero column)
  0x7fffffff entries         every image of at most 960 rows (idle waves in the LDS combine)

Mutants of oicr_targets_body (each built alone on a scratch copy; test_oicr_targets_equals_reference cases that fail):
  a  wave combine `oi > bi`                        rows-2, rows-63, rows-64, rows-65, ties-*
  b  LDS combine `si[g][q] > bi`                   rows-65, ties-*
  c  sv / si indexed by k instead of g0 + k        every case with G > 4 (34); run with the reader on `g & 3`, so that no
                                                   unwritten LDS slot became a row index
  d  `best > lo`                                   exact-thr2, exact-thr3  (at (0.5,), (0, 1) a row on the threshold falls in no
                                                   interval and keeps the Matcher's default label 1, which is labels[1])
  e  `iou >= best`                                 63 tests: every case with two mined boxes, ioutie, ioutie-reversed
  f  class offset 0 instead of 4 * cls             K80-G80, 4K-K5, 4K-K20, empty-last-4K
  g  third labelling loop from + 3072              every case with an image above 2048 rows (13)
  h  cx = fma(0.5, w, b0) in the zero-delta decode decode-subnormal only: 0.5f * w is exact for every normal w, so the fused
                                                   and the unfused form differ only where it underflows
  i  vb's value select without `r + 1024 < r1`     none, and none can: the update two lines below repeats the guard, so the
                                                   selected value is never used (an equivalent mutant)
The kernel before this suite's two fixes fails G0-lab0-ignore and all six empty-* cases."""
import ctypes

import numpy as np
import pytest
import torch

import oicr_targets_util as U
from __graft_entry__ import load_package
from test_ops_gpu import _boxes, _mil_equals_separate

pytestmark = pytest.mark.gpu
DEV = "cuda"
FILL, SPARE_BOX, SPARE_SCORE = -77, 77777.0, 9.0
KEYS = ("labels", "matched", "weights", "gt_boxes")


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


def _with_spare_row(x, value):
    buf = torch.full((x.shape[0] + 1,) + tuple(x.shape[1:]), value, dtype=torch.float32)
    buf[: x.shape[0]] = torch.from_numpy(x)
    return buf.to(DEV)


def _inputs(case):
    """device inputs of one case: the first M rows of buffers one row longer; bg == 2: prev_scores is a column window"""
    M, K, n_img, gmax = len(case["props"]), case["K"], len(case["M_per"]), case["gmax"]
    prev = case["prev"]
    if case["bg"] == 2:
        wide = np.full((M, prev.shape[1] + 5), SPARE_SCORE, dtype=np.float32)
        wide[:, 2: 2 + prev.shape[1]] = prev
        scores = _with_spare_row(wide, SPARE_SCORE)[:M, 2: 2 + prev.shape[1]]
        assert scores.stride(0) > K + 1
    else:
        scores = _with_spare_row(prev, SPARE_SCORE)[:M]
    props = _with_spare_row(case["props"], SPARE_BOX)[:M]
    pb = props if case["boxes"] != "4K" else _with_spare_row(case["prev_boxes"], SPARE_BOX)[:M]
    gcl = torch.full((n_img, gmax), K - 1, dtype=torch.int32)  # slots from G_i on: a valid class the kernel must not use
    for i, g in enumerate(case["gts"]):
        gcl[i, : len(g)] = torch.tensor(g, dtype=torch.int32)
    gcn = torch.tensor([len(g) for g in case["gts"]], dtype=torch.int32)
    return dict(scores=scores, props=props, pb=pb, off=torch.tensor(case["off"], dtype=torch.int32, device=DEV),
                gcl=gcl.to(DEV), gcn=gcn.to(DEV), img_scores=torch.from_numpy(case["img_scores"]).to(DEV))


def _outputs(M, n_img, gmax, extra=3):
    f = lambda shape, dt: torch.full(shape, FILL, dtype=dt, device=DEV)
    return dict(labels=f((M + extra,), torch.int32), weights=f((M + extra,), torch.float32),
                matched=f((M + extra,), torch.int32), gt_boxes=f((M + extra, 4), torch.float32),
                pgt_idx=f((n_img + 1, gmax), torch.int32), pgt_boxes=f((n_img + 1, gmax, 4), torch.float32))


def _cat(ref, key):
    return torch.from_numpy(np.concatenate([r[key] for r in ref], 0))


def _assert_equals_ref(out, case, ref, tag=""):
    """labels / matched / weights / gt_boxes of every row, pgt_idx / pgt_boxes of the first G_i slots of every image"""
    M = len(case["props"])
    for key in KEYS:
        got = out[key][:M].cpu()
        assert torch.equal(got.long() if got.dtype == torch.int32 else got, _cat(ref, key)), (tag, case["id"], key)
    for i, r in enumerate(ref):
        g = len(case["gts"][i])
        assert torch.equal(out["pgt_idx"][i, :g].cpu().long(), torch.from_numpy(r["pgt_idx"])), (tag, case["id"], i)
        assert torch.equal(out["pgt_boxes"][i, :g].cpu(), torch.from_numpy(r["pgt_boxes"])), (tag, case["id"], i)


@pytest.mark.parametrize("cid", U.case_ids())
def test_oicr_targets_equals_reference(drn, cid):
    case, ref = U.case_by_id(cid), U.refs()[cid]
    M, n_img = len(case["props"]), len(case["M_per"])
    b, out = _inputs(case), _outputs(len(case["props"]), len(case["M_per"]), case["gmax"])
    res = drn.oicr_targets(b["scores"], b["pb"], b["props"], b["off"], n_img, b["gcl"], b["gcn"], b["img_scores"],
                           case["K"], case["thr"], case["lab"], zero_delta_decode=case["decode"], out=out)
    assert res is out
    _assert_equals_ref(out, case, ref)
    # rows of no image and the pseudo-GT slots of no image: untouched
    for key in KEYS:
        assert bool((out[key][M:] == FILL).all()), key
    assert bool((out["pgt_idx"][n_img] == FILL).all()) and bool((out["pgt_boxes"][n_img] == FILL).all())
    # nothing of the spare input row in any output (an image without proposals in last place reads there if it reads)
    for key in ("gt_boxes", "pgt_boxes"):
        assert not bool((out[key] == SPARE_BOX).any()), key


REFUSALS = [dict(gmax=0), dict(gmax=129), dict(nthr=0), dict(nthr=4), dict(box_cols=8), dict(box_cols=12),
            dict(box_cols=4 * 20, zero_delta_decode=1)]


@pytest.mark.parametrize("bad", REFUSALS, ids=lambda d: "-".join("%s%d" % kv for kv in sorted(d.items())))
def test_oicr_targets_refusals(drn, cabi, bad):
    """arguments outside the kernel's class: the argument error, and no output written"""
    case = U.case_by_id("4K-K20") if bad.get("box_cols") == 80 else U.case_by_id("rows-65")
    M, n_img, K = len(case["props"]), len(case["M_per"]), case["K"]
    b, out = _inputs(case), _outputs(M, n_img, 129)
    a = dict(gmax=case["gmax"], nthr=1, box_cols=b["pb"].shape[1], zero_delta_decode=0)
    a.update(bad)
    th, lb = cabi.host_floats((0.2, 0.4, 0.6, 0.8)), cabi.host_ints((0, 1, 0, 1, 0))
    vp = lambda x: ctypes.cast(x, ctypes.c_void_p)
    P = cabi.ptr
    with pytest.raises(cabi.DrnError, match="invalid argument"):
        cabi.call("drn_oicr_targets", P(b["scores"]), b["scores"].stride(0), P(b["pb"]), a["box_cols"], a["zero_delta_decode"],
                  P(b["props"]), P(b["off"]), n_img, P(b["gcl"]), P(b["gcn"]), a["gmax"], P(b["img_scores"]), K, vp(th),
                  vp(lb), a["nthr"], P(out["labels"]), P(out["weights"]), P(out["matched"]), P(out["gt_boxes"]),
                  P(out["pgt_idx"]), P(out["pgt_boxes"]), cabi.stream())
    torch.cuda.synchronize()
    for key, t in out.items():
        assert bool((t == FILL).all()), key


# ------------------------------------------------------------------------------------------- the multi-head launches
def _chain_inputs(K, M_per, nh, draws, gmax, seed=77):
    M, n_img = sum(M_per), len(M_per)
    rs = np.random.RandomState(seed)
    C_ = K + 1
    ld = 2 * K + nh * C_ + 5
    col0s = [2 * K + k * C_ for k in range(nh)]
    logits = torch.from_numpy(rs.standard_normal((M, ld)).astype(np.float32) * 3)
    scores0 = rs.rand(M, K).astype(np.float32)
    props = _boxes(M, 33)
    img_scores = rs.rand(n_img, K).astype(np.float32)
    gts = [[int(c) for c in rs.permutation(K)[: 1 + rs.randint(draws)]] for _ in range(n_img)]
    gts[0] = [int(c) for c in rs.permutation(K)[:draws]]  # the first image holds the largest count
    return dict(K=K, M_per=list(M_per), off=[0] + [int(x) for x in np.cumsum(M_per)], gts=gts, gmax=gmax, nh=nh, ld=ld,
                col0s=col0s, logits=logits, prev=scores0, props=props.numpy(), prev_boxes=props.numpy(),
                img_scores=img_scores, bg=0, boxes="props", decode=False, thr=(0.5,), lab=(0, 1), id="chain")


CHAIN_SHAPES = [(20, [2049, 31], 3, 9, 16), (80, [4097], 2, 17, 32), (6, [1025, 0, 1023], 8, 5, 8)]


@pytest.mark.parametrize("K,M_per,nh,draws,gmax", CHAIN_SHAPES)
def test_oicr_refine_chain_equals_per_head_sequence_and_reference(drn, K, M_per, nh, draws, gmax):
    """drn_oicr_refine_chain == targets -> softmax-CE per head, bit for bit, with more than four classes, rows past 2048
    and up to MAX_CHAIN_HEADS heads; head 0, whose scores are a given input, also == the reference (so the
    blockIdx.y dispatch is tied to the oracle and not only to the single-head kernel)"""
    c = _chain_inputs(K, M_per, nh, draws, gmax)
    M, n_img, C_ = sum(M_per), len(M_per), K + 1
    assert max(len(g) for g in c["gts"]) == draws > 4 and max(M_per) > 1024
    b = _inputs(c)
    logits = c["logits"].to(DEV)
    dl_a = torch.zeros((M, c["ld"]), device=DEV)
    dl_b = torch.zeros((M, c["ld"]), device=DEV)
    chain = drn.oicr_refine_chain(logits, c["col0s"], K, b["scores"], b["props"], b["off"], n_img, b["gcl"], b["gcn"],
                                  b["img_scores"], dlogits=dl_a)
    _assert_equals_ref(chain[0][0], c, U.case_ref(c), "head 0")
    prev, zero = b["scores"], False
    for k in range(nh):
        tg = drn.oicr_targets(prev, b["props"], b["props"], b["off"], n_img, b["gcl"], b["gcn"], b["img_scores"], K,
                              zero_delta_decode=zero)
        probs, loss = drn.softmax_ce(logits, c["col0s"][k], C_, tg["labels"], tg["weights"], dlogits=dl_b)
        ctg, cprobs, closs = chain[k]
        for key in KEYS:
            assert torch.equal(ctg[key], tg[key]), (k, key)
        for i in range(n_img):  # only the first G_i mined entries per image are defined
            g = len(c["gts"][i])
            assert torch.equal(ctg["pgt_idx"][i, :g], tg["pgt_idx"][i, :g]), (k, i)
            assert torch.equal(ctg["pgt_boxes"][i, :g], tg["pgt_boxes"][i, :g]), (k, i)
        assert torch.equal(cprobs, probs) and torch.equal(closs, loss), k
        prev, zero = probs, True
    assert torch.equal(dl_a, dl_b)
    assert float(dl_a.abs().max()) > 0


@pytest.mark.parametrize("K,M_per,nh,draws,gmax", CHAIN_SHAPES)
def test_mil_oicr_losses_equals_separate_calls_many_classes(drn, K, M_per, nh, draws, gmax):
    """drn_mil_oicr_losses == the separate calls (test_ops_gpu._mil_equals_separate, unchanged in what it asserts) with
    up to `draws` classes per image in gmax slots"""
    _mil_equals_separate(drn, K, M_per, nh, 5, True, gmax=gmax, draws=draws)
