"""The reference of test_oicr_targets_gpu.py (oicr_targets_util.py) against oracle/wsod_oracle.py, bit for bit on every case
where the oracle is defined, and the case table against what it claims: planted ties are bit-equal maxima, the exact IoUs
equal their thresholds in fp32, every Matcher interval and label value is hit, and every code path of the kernel that the
suite is built around is reached by at least one case (pytest -s prints the case ids per path)."""
import numpy as np
import pytest
import torch

import oicr_targets_util as U

F32 = np.float32


@pytest.mark.parametrize("cid", U.case_ids())
def test_reference_equals_oracle(cid):
    case, ref = U.case_by_id(cid), U.refs()[cid]
    orc = U.oracle_targets(case)
    for i, (r, o) in enumerate(zip(ref, orc)):
        n, g = case["M_per"][i], len(case["gts"][i])
        for key in ("labels", "matched", "weights", "gt_boxes", "pgt_idx", "pgt_boxes"):
            assert r[key].shape[0] == (g if key.startswith("pgt") else n), (i, key)  # no row and no slot is exempt
        if o is None:  # the oracle has no value for an image without proposals: the reference defines it
            assert n == 0 and not r["pgt_idx"].any() and not r["pgt_boxes"].any()
            continue
        for key in ("labels", "matched", "weights", "gt_boxes", "pgt_idx", "pgt_boxes"):
            assert torch.equal(torch.from_numpy(r[key]), o[key]), (i, key)
        if g == 0:
            assert (r["labels"] == case["K"]).all() and not r["weights"].any() and not r["gt_boxes"].any()


def test_zero_delta_decode_equals_oracle_and_moves_boxes():
    """apply_deltas(0, b) in numpy == the oracle's, bit for bit, and it is not the identity (so a kernel that skipped the
    decode, or rounded it differently, would show)"""
    props = U.case_by_id("rows-5000")["props"]
    dec = U.apply_zero_deltas_ref(props)
    assert torch.equal(torch.from_numpy(dec), U.O.apply_deltas(torch.zeros((len(props), 4)), torch.from_numpy(props)))
    assert (dec != props).any(1).sum() > len(props) // 10
    sub = U.apply_zero_deltas_ref(np.array([[U.SUB, U.SUB, 2 * U.SUB, 2 * U.SUB]], dtype=F32))
    assert (sub == F32(U.SUB)).all()  # 0.5 * w underflows to 0; a fused b0 + 0.5 * w would give 2 * SUB


@pytest.mark.parametrize("cid", U.case_ids())
def test_planted_maxima_and_ties(cid):
    case, ref = U.case_by_id(cid), U.refs()[cid]
    for img, cls, rows in case["ties"]:
        r0, n = case["off"][img], case["M_per"][img]
        col = case["prev"][r0: r0 + n, cls]
        assert all(col[r].tobytes() == col.max().tobytes() for r in rows), (img, cls)  # bit-equal maxima
        assert int((col == col.max()).sum()) == len(rows)  # and no other row holds it
        if cls in case["gts"][img]:
            assert int(ref[img]["pgt_idx"][case["gts"][img].index(cls)]) == min(rows)
    if case["boxes"] == "4K":  # every class copy of a row differs: a wrong 4 * cls offset cannot pass
        b = case["prev_boxes"].reshape(len(case["props"]), case["K"], 4)
        assert all((b[:, k] != b[:, j]).any(1).all() for k in range(case["K"]) for j in range(k))
    if case["id"] == "decode-subnormal":
        assert (ref[0]["pgt_boxes"][0] == F32(U.SUB)).all() and (case["props"][5, 2:] == F32(2 * U.SUB)).all()


@pytest.mark.parametrize("j", range(len(U.MATCHERS)))
def test_exact_ious_and_matcher_intervals(j):
    thr, lab = U.MATCHERS[j]
    case = U.case_by_id("exact-thr%d" % len(thr))
    ref = U.refs()[case["id"]][0]
    assert (case["thr"], case["lab"]) == (thr, lab)
    assert int(ref["pgt_idx"][0]) == 17 and ref["pgt_boxes"][0].tolist() == U.BOX_A
    on_threshold = set()
    for k, (box, inter, union) in enumerate(U.EXACT):
        row = 20 + k
        v = F32(inter) / F32(union)
        assert case["props"][row].tolist() == box
        assert pairwise32(ref, 0, row, case) == v and abs(ref["iou64"][0, row] - inter / union) < 1e-15
        assert ref["best_iou"][row] == v  # no other mined box reaches the planted corner
        assert int(ref["matched"][row]) == 0
        for t in thr:
            if v == F32(t):
                on_threshold.add(t)
                q = list(thr).index(t) + 1  # >= lo: the row is in the interval that STARTS at the threshold
                want = {0: case["K"], -1: -1, 1: case["gts"][0][0]}[lab[q]]
                assert int(ref["labels"][row]) == want
                assert float(ref["weights"][row]) == (0.0 if want == -1 else float(case["img_scores"][0, case["gts"][0][0]]))
    assert on_threshold == set(thr)  # every threshold constant is met exactly by one planted row
    # every interval and every label value is hit
    edges = [-np.inf] + [F32(t) for t in thr] + [np.inf]
    for q in range(len(lab)):
        assert ((ref["best_iou"] >= edges[q]) & (ref["best_iou"] < edges[q + 1])).any(), q
    got = set(ref["labels"].tolist())
    assert case["K"] in got and (-1 in got) == (-1 in lab) and got & set(case["gts"][0])
    assert (ref["weights"][ref["labels"] == -1] == 0).all()


def pairwise32(ref, g, row, case):
    return U.pairwise_iou_ref(ref["pgt_boxes"][g: g + 1], case["props"][row: row + 1])[0, 0]


def test_iou_tie_between_two_mined_boxes():
    for cid in ("ioutie", "ioutie-reversed"):
        case, (ref,) = U.case_by_id(cid), U.refs()[cid]
        a, b = (U.BOX_A, U.BOX_B) if cid == "ioutie" else (U.BOX_B, U.BOX_A)
        assert ref["pgt_boxes"].tolist() == [a, b]
        i0, i1 = pairwise32(ref, 0, 12, case), pairwise32(ref, 1, 12, case)
        assert i0.tobytes() == i1.tobytes() and i0 == F32(50) / F32(150)
        assert int(ref["matched"][12]) == 0 and ref["gt_boxes"][12].tolist() == a
        assert int(ref["labels"][12]) == -1  # 1/3 lies in [0.3, 0.7)


def test_empty_and_no_gt_cases():
    c = U.case_by_id("G0-lab0-ignore")
    assert c["lab"][0] == -1 and c["gts"][0] == [] and (U.refs()[c["id"]][0]["labels"] == c["K"]).all()
    where = set()
    for c in U.cases():
        for i, n in enumerate(c["M_per"]):
            if n == 0 and len(c["gts"][i]) > 0:
                where.add("first" if i == 0 else "last" if i == len(c["M_per"]) - 1 else "middle")
    assert where == {"first", "middle", "last"}
    assert sum(n > 0 for n in U.case_by_id("empty-all-but-one")["M_per"]) == 1


def test_every_code_path_is_reached():
    reach = {p: [] for p in U.PATHS}
    for c in U.cases():
        for p in U.paths(c, U.refs()[c["id"]]):
            reach[p].append(c["id"])
    for p in U.PATHS:
        print("PATH %-13s %s" % (p, " ".join(reach[p])))
        assert reach[p], p
    # the table holds the sizes, class counts, layouts and box modes it was written for
    rows = {n for c in U.cases() for n in c["M_per"]}
    assert {1, 2, 63, 64, 65, 1023, 1024, 1025, 2047, 2048, 2049, 3071, 3073, 4097, 5000} <= rows
    assert {(len(g), c["gmax"]) for c in U.cases() for g in c["gts"]} >= {(g, m) for g in (1, 3, 4, 5, 7, 8, 9, 17)
                                                                        for m in (g, g + 3, 32)} | {(80, 80), (128, 128)}
    assert {(c["boxes"], c["bg"]) for c in U.cases()} >= {(b, s) for b in ("props", "decode") for s in (0, 1, 2)}
    assert {c["K"] for c in U.cases() if c["boxes"] == "4K"} >= {5, 20, 80}
    assert {(c["thr"], c["lab"]) for c in U.cases()} >= set(U.MATCHERS)
    assert any(sorted(g) != g for c in U.cases() for g in c["gts"])  # unsorted class lists
