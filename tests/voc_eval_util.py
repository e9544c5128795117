"""Test infrastructure of the device-side PASCAL VOC evaluator: a plain numpy fp64 restatement of the evaluator with the
stable tie definition - the host algorithm of evaluation.py (voc_eval, voc_eval_corloc, voc_ap, _max_overlap) with
np.argsort(-conf, kind="stable") over the lines kept in processing order, quantising by formula instead of through text
- and the builders of the cases the CPU and GPU tests share.

A case is a dict:
  classes   [K] names
  annos     {image_id: [(class name, difficult, [xmin, ymin, xmax, ymax])]}   (what the evaluator takes)
  calls     [(image_id, boxes [m, 4] f32 XYXY 0-based, scores [m] f32, classes [m] i64)]   one process() call each, in order"""
import numpy as np

THRS = np.array([t / 100.0 for t in range(50, 100, 5)], np.float64)  # the evaluator's thr / 100.0
REC_THRS = np.arange(0.0, 1.1, 0.1)  # voc_ap's own expression


def quant_score(s):
    """float("%.3f" % s) for float32 s, by formula (exact product, half-to-even rint, correctly rounded division)"""
    assert s.dtype == np.float32
    return np.rint(s.astype(np.float64) * 1000.0) / 1000.0 + 0.0  # + 0.0: -0.0 -> +0.0


def quant_box(b):
    """the four numbers format_prediction prints for a float32 XYXY box: the +1 of xmin / ymin is a float32 add"""
    assert b.dtype == np.float32
    b = b.reshape(-1, 4).copy()
    b[:, :2] = b[:, :2] + np.float32(1)
    return np.rint(b.astype(np.float64) * 10.0) / 10.0


def max_overlap(bb, BBGT):
    if BBGT.size == 0:
        return -np.inf, -1
    iw = np.maximum(np.minimum(BBGT[:, 2], bb[2]) - np.maximum(BBGT[:, 0], bb[0]) + 1.0, 0.0)
    ih = np.maximum(np.minimum(BBGT[:, 3], bb[3]) - np.maximum(BBGT[:, 1], bb[1]) + 1.0, 0.0)
    inters = iw * ih
    uni = ((bb[2] - bb[0] + 1.0) * (bb[3] - bb[1] + 1.0) + (BBGT[:, 2] - BBGT[:, 0] + 1.0) * (BBGT[:, 3] - BBGT[:, 1] + 1.0)
           - inters)
    ov = inters / uni
    return np.max(ov), int(np.argmax(ov))


def voc_ap(rec, prec, use_07_metric):
    if use_07_metric:
        ap = 0.0
        for t in REC_THRS:
            p = 0 if np.sum(rec >= t) == 0 else np.max(prec[rec >= t])
            ap = ap + p / 11.0
        return ap
    mrec = np.concatenate(([0.0], rec, [1.0]))
    mpre = np.concatenate(([0.0], prec, [0.0]))
    for i in range(mpre.size - 1, 0, -1):
        mpre[i - 1] = np.maximum(mpre[i - 1], mpre[i])
    i = np.where(mrec[1:] != mrec[:-1])[0]
    return np.sum((mrec[i + 1] - mrec[i]) * mpre[i + 1])


def flat_inputs(case):
    """the arrays ops.voc_match / ops.voc_accumulate take: detections in processing order, ground truth grouped by
    (image, class) pair in annotation order, per class npos / npos_im"""
    names, annos = case["classes"], case["annos"]
    K, ids = len(names), list(annos)
    I = len(ids)
    index = {iid: i for i, iid in enumerate(ids)}
    gt_box, gt_diff, off = [], [], [0]
    npos, npos_im = np.zeros(K, np.int32), np.zeros(K, np.int32)
    for iid in ids:
        for k, name in enumerate(names):
            R = [o for o in annos[iid] if o[0] == name]
            gt_box += [o[2] for o in R]
            gt_diff += [1 if o[1] else 0 for o in R]
            off.append(off[-1] + len(R))
            easy = sum(1 for o in R if not o[1])
            npos[k] += easy
            npos_im[k] += min(1, easy)
    calls = case["calls"]
    if calls:
        cat = lambda j, dt, shape: np.concatenate([np.asarray(c[j], dt).reshape(shape) for c in calls])
        box, score, cls = cat(1, np.float32, (-1, 4)), cat(2, np.float32, (-1,)), cat(3, np.int64, (-1,))
        img = np.concatenate([np.full(len(c[2]), index[c[0]], np.int64) for c in calls])
    else:
        box, score = np.zeros((0, 4), np.float32), np.zeros(0, np.float32)
        cls, img = np.zeros(0, np.int64), np.zeros(0, np.int64)
    return dict(I=I, K=K, det_box=box, det_score=score, det_cls=cls, det_img=img, det_pair=(img * K + cls).astype(np.int32),
                gt_box=np.array(gt_box, np.float64).reshape(-1, 4), gt_diff=np.array(gt_diff, np.uint8),
                gt_off=np.array(off, np.int32), npos=npos, npos_im=npos_im)


def restate(case, thrs=THRS):
    """-> per class k a dict: order (indices into the processing-order detections), score (quantised, ranked), ovmax,
    jmax [nd], tp / fp [T, nd] (flags), rec / prec [T, nd], ap07 / ap12 / corloc [T]"""
    f = flat_inputs(case)
    K, T = f["K"], len(thrs)
    qs, qb = quant_score(f["det_score"]), quant_box(f["det_box"])
    out = []
    for k in range(K):
        idx = np.nonzero(f["det_cls"] == k)[0]
        order = idx[np.argsort(-qs[idx], kind="stable")]
        nd = len(order)
        ovmax, jmax = np.full(nd, -np.inf), np.full(nd, -1, np.int32)
        gts = []
        for d, o in enumerate(order):
            p = int(f["det_img"][o]) * K + k
            g0, g1 = f["gt_off"][p], f["gt_off"][p + 1]
            gts.append((p, g0, g1))
            ovmax[d], jmax[d] = max_overlap(qb[o], f["gt_box"][g0:g1])
        tp, fp = np.zeros((T, nd)), np.zeros((T, nd))
        rec, prec = np.zeros((T, nd)), np.zeros((T, nd))
        ap07, ap12, corloc = np.zeros(T), np.zeros(T), np.zeros(T)
        npos, npos_im = int(f["npos"][k]), int(f["npos_im"][k])
        for ti, thr in enumerate(thrs):
            det, seen, hits = set(), set(), 0
            for d in range(nd):
                p, g0, g1 = gts[d]
                if ovmax[d] > thr:
                    if not f["gt_diff"][g0 + jmax[d]]:
                        if (p, jmax[d]) not in det:
                            tp[ti, d] = 1.0
                            det.add((p, jmax[d]))
                        else:
                            fp[ti, d] = 1.0
                else:
                    fp[ti, d] = 1.0
                if p not in seen and not all(f["gt_diff"][g0:g1]):  # CorLoc: the image's top-ranked detection decides
                    seen.add(p)
                    hits += int(ovmax[d] > thr)
            ctp, cfp = np.cumsum(tp[ti]), np.cumsum(fp[ti])
            rec[ti] = ctp / float(npos) if npos > 0 else np.zeros_like(ctp)
            prec[ti] = ctp / np.maximum(ctp + cfp, np.finfo(np.float64).eps)
            ap07[ti], ap12[ti] = voc_ap(rec[ti], prec[ti], True), voc_ap(rec[ti], prec[ti], False)
            corloc[ti] = 1.0 * hits / npos_im if nd and npos_im else 0.0
        out.append(dict(order=order, score=qs[order], ovmax=ovmax, jmax=jmax, tp=tp, fp=fp, rec=rec, prec=prec, ap07=ap07,
                        ap12=ap12, corloc=corloc))
    return out


def results_dict(case, res, year):
    """the evaluator's OrderedDict from a restatement, with the host path's arithmetic"""
    key = "ap07" if year == 2007 else "ap12"
    names = case["classes"]
    aps = {t: [r[key][ti] * 100 for r in res] for ti, t in enumerate(range(50, 100, 5))}
    cls_ = {t: [r["corloc"][ti] * 100 for r in res] for ti, t in enumerate(range(50, 100, 5))}
    m, c = {t: np.mean(x) for t, x in aps.items()}, {t: np.mean(x) for t, x in cls_.items()}
    return {"bbox": {"AP": np.mean(list(m.values())), "AP50": m[50], "AP75": m[75]},
            "bbox CorLoc": {"CL": np.mean(list(c.values())), "CL50": c[50], "CL75": c[75]},
            "per_class": {"AP50": dict(zip(names, aps[50])), "CL50": dict(zip(names, cls_[50]))}}


def host_lines(case, E):
    """{class: the host path's text lines} in processing order"""
    lines = {k: [] for k in range(len(case["classes"]))}
    for iid, box, score, cls in case["calls"]:
        for b, s, c in zip(np.asarray(box, np.float32).reshape(-1, 4), np.asarray(score, np.float32), cls):
            lines[int(c)].append(E.format_prediction(iid, s, b.copy()))
    return lines


def feed(evaluator, case, device="cpu", calls=None):
    import torch

    from drn_wsod_pytorch_amd.structures import Boxes, Instances

    for iid, box, score, cls in (case["calls"] if calls is None else calls):
        inst = Instances((500, 500))
        inst.pred_boxes = Boxes(torch.from_numpy(np.asarray(box, np.float32).reshape(-1, 4)).to(device))
        inst.scores = torch.from_numpy(np.asarray(score, np.float32)).to(device)
        inst.pred_classes = torch.from_numpy(np.asarray(cls, np.int64)).to(device)
        evaluator.process([{"image_id": iid}], [{"instances": inst}])


def assert_tie_free(case):
    f = flat_inputs(case)
    qs = quant_score(f["det_score"])
    for k in range(f["K"]):
        s = qs[f["det_cls"] == k]
        assert len(np.unique(s)) == len(s), "class %d has tied quantised scores" % k


# ---- cases ------------------------------------------------------------------------------------------------------------

def golden_case(classes, annos, dets):
    """golden_util.voc_fixture as a case: one process() call per image, detections in fixture order"""
    by_img = {}
    for c, iid, score, box in dets:
        by_img.setdefault(iid, []).append((c, score, box))
    calls = [(iid, np.array([b for _, _, b in it], np.float32), np.array([s for _, s, _ in it], np.float32),
              np.array([c for c, _, _ in it], np.int64)) for iid, it in by_img.items()]
    return dict(classes=list(classes), annos=annos, calls=calls)


def _random_annos(rng, n_img, names, max_obj=4, p_diff=0.25):
    annos = {}
    for i in range(n_img):
        objs = []
        for _ in range(int(rng.integers(0, max_obj + 1))):
            x0, y0 = int(rng.integers(1, 300)), int(rng.integers(1, 250))
            objs.append((names[int(rng.integers(len(names)))], int(rng.random() < p_diff),
                         [x0, y0, x0 + int(rng.integers(15, 150)), y0 + int(rng.integers(15, 120))]))
        annos["%06d" % (i + 1)] = objs
    return annos


def _random_boxes(rng, objs, names, m):
    """m detections: about two thirds jittered ground-truth boxes of the image (class mostly kept), the rest random"""
    box, cls = np.zeros((m, 4)), np.zeros(m, np.int64)
    for j in range(m):
        if objs and rng.random() < 0.65:
            name, _, bb = objs[int(rng.integers(len(objs)))]
            jit = rng.normal(0, 1, 4) * rng.choice([1.5, 12.0])
            box[j] = [bb[0] - 1 + jit[0], bb[1] - 1 + jit[1], bb[2] + jit[2], bb[3] + jit[3]]
            cls[j] = names.index(name) if rng.random() < 0.85 else rng.integers(len(names))
        else:
            x0, y0 = rng.random() * 300, rng.random() * 250
            box[j] = [x0, y0, x0 + rng.uniform(10, 150), y0 + rng.uniform(10, 120)]
            cls[j] = rng.integers(len(names))
    return box.astype(np.float32), cls


def tie_free_case(seed=3, n_img=60, n_cls=5, per_img=25):
    """about n_img * per_img detections whose scores are, per class, a random permutation of distinct multiples of 0.001"""
    rng = np.random.default_rng(seed)
    names = ["c%d" % k for k in range(n_cls)]
    annos = _random_annos(rng, n_img, names)
    calls = []
    for iid, objs in annos.items():
        box, cls = _random_boxes(rng, objs, names, per_img)
        calls.append([iid, box, None, cls])
    for k in range(n_cls):
        nk = sum(int((c[3] == k).sum()) for c in calls)
        vals = iter(rng.permutation(np.arange(1, 3 * nk + 1))[:nk] / 1000.0)  # distinct after %.3f; may exceed 1
        for c in calls:
            if c[2] is None:
                c[2] = np.zeros(len(c[3]), np.float32)
            for j in np.nonzero(c[3] == k)[0]:
                c[2][j] = np.float32(next(vals))
    case = dict(classes=names, annos=annos, calls=[tuple(c) for c in calls])
    assert_tie_free(case)
    return case


TIE_SCORES = np.array([0.12349, 0.1235, 0.12351, 0.0004, 0.0001, 0.00049, 0.9, 0.5, 0.5005, 0.4995, 0.75, 0.0, -0.0, 0.25],
                      np.float32)


def edge_case(seed=5, n_img=40, per_img=75):
    """tie-heavy scores from TIE_SCORES and the hand-made situations the GPU test lists.  Classes: c0 .. c2 ordinary, c3
    has no detections, c4 has no ground truth anywhere (npos = 0)"""
    rng = np.random.default_rng(seed)
    names = ["c%d" % k for k in range(5)]
    annos = _random_annos(rng, n_img, names[:3])
    ids = list(annos)
    annos[ids[0]] = [("c0", 0, [1, 1, 10, 10]), ("c3", 0, [50, 50, 90, 90])]
    annos[ids[1]] = [("c1", 1, [20, 20, 80, 90]), ("c1", 0, [20, 20, 80, 90]), ("c2", 0, [20, 20, 80, 90]),
                     ("c2", 1, [20, 20, 80, 90])]  # identical boxes, (difficult, not) in both orders: first-index argmax
    annos[ids[2]] = [("c0", 1, [30, 30, 100, 100]), ("c0", 1, [120, 40, 200, 160])]  # every box of the class difficult
    annos[ids[3]] = []  # detections, no ground truth
    calls = []
    for n, (iid, objs) in enumerate(annos.items()):
        box, cls = _random_boxes(rng, objs, names, per_img)
        cls[cls == 3] = 0  # c3 keeps its ground truth and gets no detection
        cls[rng.random(per_img) < 0.1] = 4  # the class without ground truth still gets detections
        box = np.round(box * 4) / 4  # quarter pixels: .25 / .75 are %.1f ties, exact in binary
        score = TIE_SCORES[rng.integers(0, len(TIE_SCORES), per_img)]
        if n == 0:
            # IoU exactly 0.5 with [1, 1, 10, 10]: prints as [1, 1, 10, 5] -> 50 / 100, no match at 0.5 (strict >); then a
            # better box twice (the second is a false positive); then boxes left of / above the GT (iw, ih < 0 unclamped)
            box[:6] = [[0, 0, 10, 5], [0, 0, 10, 9], [0, 0, 10, 9], [200, 0, 260, 9], [0, 300, 9, 380], [9.25, 9.75, 30.25, 40.75]]
            cls[:6] = 0
            score[:6] = [1.5, 1.25, 1.25, 1.0, 1.0, 0.95]  # ahead of every random detection
        if n == 1:
            box[:4] = [[19, 19, 80, 90], [19, 19, 80, 90], [19, 19, 80, 90], [19, 19, 80, 90]]
            cls[:4] = [1, 1, 2, 2]
            score[:4] = [1.5, 1.25, 1.5, 1.25]
        if n == 2:
            box[:2] = [[29, 29, 100, 100], [119, 39, 200, 160]]
            cls[:2] = 0
        calls.append((iid, box.astype(np.float32), score.astype(np.float32), cls))
    return dict(classes=names, annos=annos, calls=calls)


def tile_case(seed=9, n_big=2 * 4096 + 37, n_img=12):
    """one class with n_big detections over several images (the radix sort's tiles hold 4096) and heavy ties, plus a
    second small class"""
    rng = np.random.default_rng(seed)
    names = ["big", "small"]
    annos = _random_annos(rng, n_img, names, max_obj=6, p_diff=0.2)
    ids = list(annos)
    share = np.diff(np.linspace(0, n_big, n_img + 1).astype(np.int64))
    calls = []
    for iid, m in zip(ids, share):
        box, _ = _random_boxes(rng, annos[iid], names, int(m) + 3)
        cls = np.concatenate([np.zeros(int(m), np.int64), np.ones(3, np.int64)])
        score = (rng.integers(0, 40, int(m) + 3) / 40.0 + rng.choice([0.0, 0.0004], int(m) + 3)).astype(np.float32)
        calls.append((iid, box, score, cls))
    return dict(classes=names, annos=annos, calls=calls)


def cap_case(n_gt, seed=11):
    """n_gt boxes of one class in one image (a 16-wide grid of 12 px boxes), some difficult, and detections on them"""
    rng = np.random.default_rng(seed)
    names = ["a", "b"]
    objs = [("b", int(rng.random() < 0.2), [1 + 20 * (j % 16), 1 + 20 * (j // 16), 12 + 20 * (j % 16), 12 + 20 * (j // 16)])
            for j in range(n_gt)]
    annos = {"img7": [("a", 0, [5, 5, 60, 60])], "img9": objs}
    pick = rng.integers(0, n_gt, 300)
    box = np.array([objs[j][2] for j in pick], np.float64) + rng.integers(-2, 3, (300, 4)) - [1, 1, 0, 0]
    score = (rng.integers(0, 50, 300) / 50.0).astype(np.float32)
    calls = [("img9", box.astype(np.float32), score, np.ones(300, np.int64)),
             ("img7", np.array([[4, 4, 60, 60]], np.float32), np.array([0.5], np.float32), np.zeros(1, np.int64))]
    return dict(classes=names, annos=annos, calls=calls)
