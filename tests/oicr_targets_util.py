"""Reference and case table of drn_oicr_targets (pseudo-GT mining + proposal labelling, csrc/head.hip oicr_targets_body),
shared by test_oicr_targets_cpu.py (reference == oracle, and the cases hold what they claim) and test_oicr_targets_gpu.py
(kernel == reference, torch.equal on everything: there is no tolerance in this suite).

The kernel, for one image of n rows and G ground-truth classes (blocks of 1024 threads = 16 waves, one block per image):
  mining     four class columns per trip (g0 = 0, 4, ..; a ragged last trip clamps the class slot to G - 1); thread t reads
             rows t and t + 1024 (va / vb), then t + 2048 and t + 3072, ..; the first index wins a tie in four places: the
             ascending order inside a thread, the wave shuffle, the combine of the 16 wave results in LDS, and the
             0x7fffffff index of a thread or wave that saw no row
  labelling  rows t and t + 1024 from registers, then a third loop from t + 2048 in steps of 1024
The case table below is built around these edges; `paths(case, ref)` says which of them a case reaches.

Reference: plain numpy, every box / IoU operation in fp32 in the order oracle/wsod_oracle.py uses (pairwise_iou, matcher,
get_pgt, label_proposals, apply_deltas with all-zero deltas); np.argmax keeps the first index on ties by definition.  It
also defines the two cases the oracle cannot express:
  G == 0                        labels K, matched 0, weights 0, boxes 0 (the oracle's / the reference's has_gt == False
                                branch, whatever the Matcher's labels[0] is)
  an image without proposals    no rows; the image's first G pseudo-GT slots are index 0 and an all-zero box
The float64 IoU it returns is used only to assert properties of the cases, never as a tolerance."""
import functools

import numpy as np
import torch

import golden_util as G

O = G.O
F32 = np.float32
SUB = float(np.ldexp(1.0, -149))  # the smallest fp32 subnormal


# ------------------------------------------------------------------------------------------- reference (numpy, fp32)
def apply_zero_deltas_ref(b):
    """Box2BoxTransform.apply_deltas(zeros, b), op for op in fp32: dx = 0 / wx = 0, exp(min(0 / ww, clamp)) = 1"""
    b = np.asarray(b, dtype=F32)
    half, zero, one = F32(0.5), F32(0.0), F32(1.0)
    w, h = b[:, 2] - b[:, 0], b[:, 3] - b[:, 1]
    cx, cy = b[:, 0] + half * w, b[:, 1] + half * h
    pcx, pcy = zero * w + cx, zero * h + cy
    pw, ph = one * w, one * h
    return np.stack([pcx - half * pw, pcy - half * ph, pcx + half * pw, pcy + half * ph], 1).astype(F32)


def pairwise_iou_ref(t, p, dtype=F32):
    """t [G, 4] against p [R, 4] -> [G, R]"""
    t, p = np.asarray(t, dtype=dtype), np.asarray(p, dtype=dtype)
    a1 = (t[:, 2] - t[:, 0]) * (t[:, 3] - t[:, 1])
    a2 = (p[:, 2] - p[:, 0]) * (p[:, 3] - p[:, 1])
    wh = np.minimum(t[:, None, 2:], p[None, :, 2:]) - np.maximum(t[:, None, :2], p[None, :, :2])
    wh = np.maximum(wh, dtype(0))
    inter = wh[..., 0] * wh[..., 1]
    with np.errstate(invalid="ignore", divide="ignore"):
        return np.where(inter > 0, inter / (a1[:, None] + a2[None, :] - inter), dtype(0)).astype(dtype)


def matcher_ref(iou, thresholds, labels):
    th = [F32(-np.inf)] + [F32(t) for t in thresholds] + [F32(np.inf)]
    vals, matches = iou.max(0), iou.argmax(0)
    out = np.ones(matches.shape, dtype=np.int64)
    for l, lo, hi in zip(labels, th[:-1], th[1:]):
        out[(vals >= lo) & (vals < hi)] = l
    return matches.astype(np.int64), out, vals


def oicr_targets_ref(prev_scores, prev_boxes, props, M_per, gts, img_scores, K, thresholds=(0.5,), labels=(0, 1),
                     zero_delta_decode=False):
    """-> one dict per image: labels [n] i64, matched [n] i64, weights [n] f32, gt_boxes [n, 4] f32, pgt_idx [G] i64,
    pgt_boxes [G, 4] f32, and for the case checks best_iou [n] f32 and iou64 [G, n] f64"""
    prev_scores, prev_boxes, props = (np.asarray(x, dtype=F32) for x in (prev_scores, prev_boxes, props))
    img_scores = np.asarray(img_scores, dtype=F32)
    out, r0 = [], 0
    for i, n in enumerate(M_per):
        g = np.asarray(gts[i], dtype=np.int64)
        ps, pb, pr = prev_scores[r0: r0 + n], prev_boxes[r0: r0 + n], props[r0: r0 + n]
        r0 += n
        d = dict(labels=np.full((n,), K, dtype=np.int64), matched=np.zeros((n,), dtype=np.int64),
                 weights=np.zeros((n,), dtype=F32), gt_boxes=np.zeros((n, 4), dtype=F32),
                 pgt_idx=np.zeros((len(g),), dtype=np.int64), pgt_boxes=np.zeros((len(g), 4), dtype=F32),
                 best_iou=np.zeros((n,), dtype=F32), iou64=np.zeros((len(g), n)))
        out.append(d)
        if n == 0 or len(g) == 0:
            continue
        idx = ps[:, g].argmax(0)
        if pb.shape[1] == 4:
            boxes = (apply_zero_deltas_ref(pb) if zero_delta_decode else pb)[idx]
        else:
            boxes = np.stack([pb[idx[j], 4 * g[j]: 4 * g[j] + 4] for j in range(len(g))], 0)
        iou = pairwise_iou_ref(boxes, pr)
        matched, ml, vals = matcher_ref(iou, thresholds, labels)
        gc = g[matched].copy()
        gc[ml == 0] = K
        gc[ml == -1] = -1
        w = img_scores[i, g][matched].copy()
        w[gc == -1] = 0
        d.update(labels=gc, matched=matched, weights=w, gt_boxes=boxes[matched], pgt_idx=idx.astype(np.int64),
                 pgt_boxes=boxes, best_iou=vals, iou64=pairwise_iou_ref(boxes, pr, np.float64))
    return out


def oracle_targets(case):
    """the same through oracle/wsod_oracle.py, for every image where the oracle is defined (None for an image without
    proposals: torch.max over no rows has no value)"""
    K, M_per = case["K"], case["M_per"]
    cfg = O.OracleCfg(num_classes=K, iou_thresholds=tuple(case["thr"]), iou_labels=tuple(case["lab"]))
    prev, props = torch.from_numpy(case["prev"]), torch.from_numpy(case["props"])
    pb = torch.from_numpy(case["prev_boxes"])
    if case["decode"]:
        pb = O.apply_deltas(torch.zeros((props.shape[0], 4)), pb)
    img_scores = torch.from_numpy(case["img_scores"])
    out, r0 = [], 0
    for i, n in enumerate(M_per):
        sl = slice(r0, r0 + n)
        r0 += n
        g = torch.tensor(case["gts"][i], dtype=torch.int64)
        if n == 0:
            out.append(None)
            continue
        if len(g) == 0:
            gc, matched, gb = O.label_proposals(props[sl], torch.zeros((0, 4)), g, K, cfg)
            out.append(dict(labels=gc, matched=matched, weights=torch.zeros(n), gt_boxes=gb,
                            pgt_idx=torch.zeros(0, dtype=torch.int64), pgt_boxes=torch.zeros((0, 4))))
            continue
        (b, c, s, w, idx), = O.get_pgt([pb[sl]], [prev[sl]], [g], img_scores[i: i + 1], K)
        gc, matched, gb = O.label_proposals(props[sl], b, c, K, cfg)
        wt = w[matched].clone()
        wt[gc == -1] = 0.0  # oicr_cls_loss
        out.append(dict(labels=gc, matched=matched, weights=wt, gt_boxes=gb, pgt_idx=idx, pgt_boxes=b))
    return out


# ------------------------------------------------------------------------------------------- case builders
WIN = F32(2.0)  # planted maxima: above every random score (those are below 1)
# planted boxes live in [0, 20] x [0, 20]; the random ones start at 30, so they never touch a planted one
BOX_A, BOX_B, BOX_AB = [0, 0, 10, 10], [10, 0, 20, 10], [5, 0, 15, 10]
# (box, intersection, union) against BOX_A: every quotient is one correctly rounded fp32 division of small integers
EXACT = [([0, 0, 10, 5], 50, 100), ([0, 0, 5, 5], 25, 100), ([0, 0, 10, 3], 30, 100), ([0, 0, 10, 7], 70, 100),
         ([0, 0, 10, 1], 10, 100), ([0, 0, 10, 9], 90, 100), ([0, 0, 10, 10], 100, 100), ([3, 3, 3, 8], 0, 100),
         ([12, 12, 18, 18], 0, 136)]
MATCHERS = [((0.5,), (0, 1)), ((0.3, 0.7), (0, -1, 1)), ((0.1, 0.5, 0.9), (0, -1, 0, 1))]


def _rand_boxes(rs, M):
    x0, y0 = 30 + rs.rand(M) * 1000, 30 + rs.rand(M) * 700
    return np.stack([x0, y0, x0 + 10 + rs.rand(M) * 290, y0 + 10 + rs.rand(M) * 290], 1).astype(F32)


def classes(seed, K, Gs):
    """unique, UNSORTED class lists (the kernel follows the list's order, as index_select does)"""
    rs = np.random.RandomState(1000 + seed)
    return [[int(c) for c in rs.permutation(K)[:g]] for g in Gs]


def make_case(cid, K, M_per, gts, seed, gmax=None, bg=0, boxes="props", thr=(0.5,), lab=(0, 1), plant=()):
    """bg: 0 prev_scores [M, K]; 1 [M, K + 1] (background last); 2 the same as a column window of a wider buffer.
    boxes: "props" prev_boxes = props (box_cols 4); "decode" the same with zero_delta_decode; "4K" prev_boxes [M, 4K]
    = the oracle's apply_deltas of random deltas (every class copy different).
    plant: ("win", img, cls, row) unique maximum; ("tie", img, cls, rows) the same fp32 maximum at each row;
    ("const", img, cls, value) a constant column; ("box", img, row, [x1, y1, x2, y2]) a proposal."""
    rs = np.random.RandomState(seed)
    M = sum(M_per)
    off = [0] + [int(x) for x in np.cumsum(M_per)]
    prev = rs.rand(M, K + (1 if bg else 0)).astype(F32)
    props = _rand_boxes(rs, M)
    img_scores = rs.rand(len(M_per), K).astype(F32)
    ties = []
    for p in plant:
        r0, n = off[p[1]], M_per[p[1]]
        if p[0] == "win":
            prev[r0 + p[3], p[2]] = WIN
            ties.append((p[1], p[2], (p[3],)))
        elif p[0] == "tie":
            prev[[r0 + r for r in p[3]], p[2]] = WIN
            ties.append((p[1], p[2], tuple(p[3])))
        elif p[0] == "const":
            prev[r0: r0 + n, p[2]] = F32(p[3])
            ties.append((p[1], p[2], tuple(range(n))))
        elif p[0] == "box":
            props[r0 + p[2]] = np.asarray(p[3], dtype=F32)
    if boxes == "4K":
        deltas = torch.from_numpy(rs.standard_normal((M, 4 * K)).astype(F32))
        prev_boxes = O.apply_deltas(deltas, torch.from_numpy(props)).numpy()
    else:
        prev_boxes = props
    gmax = gmax or max(1, max(len(g) for g in gts))
    assert all(len(set(g)) == len(g) <= gmax for g in gts) and boxes in ("props", "decode", "4K")
    return dict(id=cid, K=K, M_per=list(M_per), off=off, gts=gts, gmax=gmax, bg=bg, boxes=boxes, decode=boxes == "decode",
                thr=tuple(thr), lab=tuple(lab), prev=prev, props=props, prev_boxes=prev_boxes, img_scores=img_scores,
                ties=ties, plant=list(plant))


def case_ref(case):
    return oicr_targets_ref(case["prev"], case["prev_boxes"], case["props"], case["M_per"], case["gts"], case["img_scores"],
                            case["K"], case["thr"], case["lab"], case["decode"])


def tie_sites(rows):
    """which of the kernel's tie rules decide between the rows of one planted tie (row indices inside the image)"""
    rows, sites = sorted(rows), set()
    for a, b in zip(rows[:-1], rows[1:]):
        ta, tb = a % 1024, b % 1024
        if ta == tb:
            sites.add("thread-va-vb" if (b - a == 1024 and a % 2048 < 1024) else "thread-trips")
        elif ta // 64 == tb // 64:
            sites.add("wave")
        else:
            sites.add("lds")
    return sites


PATHS = ("trips", "ragged", "mine2048", "label3", "thread-va-vb", "thread-trips", "wave", "lds", "sentinel")


def paths(case, ref):
    """the kernel's code paths this case reaches: later mining trips (g0 >= 4), a ragged last trip, a mined row >= 2048,
    the third labelling loop, each tie site, and waves that saw no row (the 0x7fffffff index in the LDS combine)"""
    out = set()
    for i, n in enumerate(case["M_per"]):
        g = len(case["gts"][i])
        if n == 0 or g == 0:
            continue
        if g > 4:
            out.add("trips")
            if g % 4:
                out.add("ragged")
        if n > 2048:
            out.add("label3")
            if int(ref[i]["pgt_idx"].max()) >= 2048:
                out.add("mine2048")
        if n <= 960:
            out.add("sentinel")
    for img, cls, rows in case["ties"]:
        if cls in case["gts"][img]:
            out |= tie_sites(rows)
    return out


# ------------------------------------------------------------------------------------------- the case table
def _exact_plants(cls_a, row0=20):
    return [("win", 0, cls_a, 17), ("box", 0, 17, BOX_A)] + [("box", 0, row0 + j, b) for j, (b, _, _) in enumerate(EXACT)]


def _build_cases():
    cs = []
    modes = ("props", "decode")
    # rows per image, single image: the unique maximum of the first class at the LAST row, of the second at the first
    # row; up to 65 rows the third class column is constant (row 0 wins)
    for j, n in enumerate([1, 2, 63, 64, 65, 1023, 1024, 1025, 2047, 2048, 2049, 3071, 3073, 4097, 5000]):
        g, = classes(j, 20, [3])
        plant = [("win", 0, g[0], n - 1), ("win", 0, g[1], 0)] + ([("const", 0, g[2], 0.25)] if n <= 65 else [])
        cs.append(make_case("rows-%d" % n, 20, [n], [g], 100 + j, gmax=3 + 3 * (j % 2), bg=j % 3, boxes=modes[j % 2],
                            plant=plant))
    # batches with offsets that are no multiple of 64, G differing per image
    for j, (M_per, Gs) in enumerate([([37, 2049, 5], [2, 7, 1]), ([1025, 1023], [5, 3]), ([4097, 1, 2048], [9, 4, 6])]):
        gts = classes(20 + j, 20, Gs)
        plant = [("win", i, gts[i][-1], n - 1) for i, n in enumerate(M_per)]
        cs.append(make_case("batch-%s" % "-".join(map(str, M_per)), 20, M_per, gts, 120 + j, gmax=max(Gs) + j, bg=j % 3,
                            boxes=modes[j % 2], plant=plant))
    # planted winners at the rows where a thread changes from va to vb and from one trip to the next
    g, = classes(30, 20, [6])
    cs.append(make_case("win-4097", 20, [4097], [g], 130, gmax=9, bg=1, boxes="decode",
                        plant=[("win", 0, c, r) for c, r in zip(g, [0, 4096, 1023, 1024, 2047, 2048])]))
    # exact ties: the smaller index wins at every site; a constant column and an all-zero one (softmax underflow)
    for j, (n, bg, mode) in enumerate([(5000, 0, "props"), (4100, 2, "decode")]):
        g, = classes(31 + j, 20, [10])
        plant = [("tie", 0, g[0], (7, 1031)), ("tie", 0, g[1], (7, 2055)), ("tie", 0, g[2], (130, 131)),
                 ("tie", 0, g[3], (400, 1034)), ("tie", 0, g[4], (1030, 2050)), ("const", 0, g[5], 0.25),
                 ("const", 0, g[6], 0.0), ("tie", 0, g[7], (63, 64)), ("tie", 0, g[8], (3000, 3001, 4025)),
                 ("tie", 0, g[9], (1500, 2524))]
        cs.append(make_case("ties-%d-%s" % (n, mode), 20, [n], [g], 131 + j, gmax=10 + 3 * j, bg=bg, boxes=mode, plant=plant))
    # G and gmax: every trip count, ragged and whole last trips
    for j, Gn in enumerate([1, 3, 4, 5, 7, 8, 9, 17]):
        for q, gmax in enumerate([Gn, Gn + 3, 32]):
            g, = classes(40 + 3 * j + q, 20, [Gn])
            n = 200 + 37 * Gn + 400 * q
            cs.append(make_case("G%d-gmax%d" % (Gn, gmax), 20, [n], [g], 140 + 3 * j + q, gmax=gmax, bg=(j + q) % 3,
                                boxes=modes[(j + q) % 2], plant=[("win", 0, g[-1], n - 1)]))
    g, = classes(70, 80, [80])
    cs.append(make_case("K80-G80", 80, [2100], [g], 170, bg=1, boxes="4K", plant=[("win", 0, g[79], 2099), ("win", 0, g[40], 2048)]))
    g, = classes(71, 130, [128])
    cs.append(make_case("K130-G128", 130, [130], [g], 171, plant=[("win", 0, g[127], 129)]))
    gts = classes(72, 20, [0, 5, 9])
    cs.append(make_case("G-0-5-9", 20, [100, 70, 64], gts, 172, gmax=12, bg=1, boxes="decode"))
    # no ground truth beside labels[0] == -1: background, not "ignore"
    gts = classes(73, 20, [0, 5])
    cs.append(make_case("G0-lab0-ignore", 20, [50, 60], gts, 173, gmax=5, thr=(0.3, 0.7), lab=(-1, 0, 1)))
    # box_cols = 4K with every class copy different
    gts = classes(74, 5, [3, 5])
    cs.append(make_case("4K-K5", 5, [65, 130], gts, 174, boxes="4K", bg=2))
    g, = classes(75, 20, [7])
    cs.append(make_case("4K-K20", 20, [2049], [g], 175, boxes="4K", gmax=8, plant=[("win", 0, g[6], 2048)]))
    # Matcher intervals with IoUs exactly on the thresholds (mined box BOX_A at row 17)
    for j, (thr, lab) in enumerate(MATCHERS):
        g, = classes(76 + j, 6, [3])
        cs.append(make_case("exact-thr%d" % len(thr), 6, [200], [g], 176 + j, gmax=4, bg=j, thr=thr, lab=lab,
                            plant=_exact_plants(g[0])))
    # an IoU tie between two mined boxes: the first slot wins, whichever class it holds
    for name, g in (("ioutie", [2, 4]), ("ioutie-reversed", [4, 2])):
        cs.append(make_case(name, 6, [100], [g], 180, thr=(0.3, 0.7), lab=(0, -1, 1),
                            plant=[("win", 0, 2, 10), ("box", 0, 10, BOX_A), ("win", 0, 4, 11), ("box", 0, 11, BOX_B),
                                   ("box", 0, 12, BOX_AB)]))
    # images without proposals: first, middle, last, all but one
    for j, (name, M_per, mode) in enumerate([("empty-first", [0, 70, 33], "props"), ("empty-middle", [40, 0, 33], "decode"),
                                            ("empty-last", [40, 33, 0], "props"), ("empty-last-decode", [2049, 0], "decode"),
                                            ("empty-last-4K", [65, 0], "4K"), ("empty-all-but-one", [0, 0, 65, 0], "props")]):
        gts = classes(82 + j, 20, [2 + (i + j) % 5 for i in range(len(M_per))])
        cs.append(make_case(name, 20, M_per, gts, 182 + j, gmax=7, bg=j % 3, boxes=mode))
    # zero-delta decode of a mined box with subnormal extents: 0.5 * w underflows (ties to even), the one place where the
    # decode's rounding order can show
    g, = classes(90, 6, [2])
    cs.append(make_case("decode-subnormal", 6, [70], [g], 190, boxes="decode",
                        plant=[("win", 0, g[0], 5), ("box", 0, 5, [SUB, SUB, 2 * SUB, 2 * SUB])]))
    ids = [c["id"] for c in cs]
    assert len(set(ids)) == len(ids)
    return cs


@functools.lru_cache(maxsize=None)
def cases():
    return tuple(_build_cases())


@functools.lru_cache(maxsize=None)
def refs():
    """case id -> reference, computed once and shared; callers must not write into it"""
    return {c["id"]: case_ref(c) for c in cases()}


def case_ids():
    return [c["id"] for c in cases()]


def case_by_id(cid):
    return next(c for c in cases() if c["id"] == cid)
