"""Restatement of pycocotools' COCOeval (bbox) and lvis-api's LVISEval / LVISResults in numpy and Python float64,
loop for loop: ``_prepare``, ``computeIoU`` (maskApi.c ``bbIou``), ``evaluateImg``, ``accumulate``, ``summarize``.
Detections enter as mmdet 3.3's CocoMetric / LVISMetric write them to the results file (``xyxy2xywh`` after
``.tolist()``, ``float(score)``).  This is the oracle of wedetect_amd.det_eval; it is a test helper, not a test file.
"""
from __future__ import annotations

from collections import defaultdict

import numpy as np

AREA_RNG = [[0 ** 2, 1e5 ** 2], [0 ** 2, 32 ** 2], [32 ** 2, 96 ** 2], [96 ** 2, 1e5 ** 2]]
AREA_LBL = ["all", "small", "medium", "large"]


def _iou_thrs():
    return np.linspace(.5, 0.95, int(np.round((0.95 - .5) / .05)) + 1, endpoint=True)


def _rec_thrs():
    return np.linspace(.0, 1.00, int(np.round((1.00 - .0) / .01)) + 1, endpoint=True)


def results_list(dets):
    """mmdet results2json for bbox: one record per det, in image order then det order."""
    out = []
    for d in dets:
        boxes = np.asarray(d["bboxes"], np.float32).reshape(-1, 4)
        scores = np.asarray(d["scores"], np.float32).reshape(-1)
        cats = np.asarray(d["category_ids"]).reshape(-1)
        for i in range(scores.shape[0]):
            b = boxes[i].tolist()
            out.append(dict(image_id=int(d["image_id"]), bbox=[b[0], b[1], b[2] - b[0], b[3] - b[1]],
                            score=float(scores[i]), category_id=int(cats[i])))
    return out


def bb_iou(dt, gt, iscrowd):
    """maskApi.c bbIou: o[d][g]."""
    m, n = len(dt), len(gt)
    o = np.zeros((m, n))
    for g in range(n):
        G = gt[g]
        ga = G[2] * G[3]
        crowd = iscrowd[g]
        for d in range(m):
            D = dt[d]
            da = D[2] * D[3]
            w = min(D[2] + D[0], G[2] + G[0]) - max(D[0], G[0])
            if w <= 0:
                continue
            h = min(D[3] + D[1], G[3] + G[1]) - max(D[1], G[1])
            if h <= 0:
                continue
            i = w * h
            u = da if crowd else da + ga - i
            o[d, g] = i / u
    return o


def _iou(dt, gt, iscrowd):
    if len(dt) == 0 or len(gt) == 0:
        return []
    return bb_iou(dt, gt, iscrowd)


def _evaluate_img(gt, dt, ious, a_rng, max_det, iou_thrs, crowd_rule, nel=None):
    """evaluateImg / evaluate_img for one (image, category, area range); gt / dt lists of dicts."""
    if len(gt) == 0 and len(dt) == 0:
        return None
    for g in gt:
        g["_ignore"] = 1 if (g["ignore"] or (g["area"] < a_rng[0] or g["area"] > a_rng[1])) else 0
    gtind = np.argsort([g["_ignore"] for g in gt], kind="mergesort")
    gt = [gt[i] for i in gtind]
    dtind = np.argsort([-d["score"] for d in dt], kind="mergesort")
    dt = [dt[i] for i in dtind[0:max_det]]
    iscrowd = [int(o.get("iscrowd", 0)) if crowd_rule else 0 for o in gt]
    ious = ious[:, gtind] if len(ious) > 0 else ious
    T, G, D = len(iou_thrs), len(gt), len(dt)
    gtm = np.zeros((T, G))
    dtm = np.zeros((T, D))
    gtIg = np.array([g["_ignore"] for g in gt])
    dtIg = np.zeros((T, D))
    if not len(ious) == 0:
        for tind, t in enumerate(iou_thrs):
            for dind, d in enumerate(dt):
                iou = min([t, 1 - 1e-10])
                m = -1
                for gind, g in enumerate(gt):
                    if gtm[tind, gind] > 0 and not iscrowd[gind]:
                        continue
                    if m > -1 and gtIg[m] == 0 and gtIg[gind] == 1:
                        break
                    if ious[dind, gind] < iou:
                        continue
                    iou = ious[dind, gind]
                    m = gind
                if m == -1:
                    continue
                dtIg[tind, dind] = gtIg[m]
                dtm[tind, dind] = gt[m]["id"]
                gtm[tind, m] = d["id"]
    if nel is None:
        a = np.array([d["area"] < a_rng[0] or d["area"] > a_rng[1] for d in dt]).reshape((1, len(dt)))
    else:
        a = np.array([d["area"] < a_rng[0] or d["area"] > a_rng[1] or d["category_id"] in nel[d["image_id"]]
                      for d in dt]).reshape((1, len(dt)))
    dtIg = np.logical_or(dtIg, np.logical_and(dtm == 0, np.repeat(a, T, 0)))
    return {"dtMatches": dtm, "gtMatches": gtm, "dtScores": [d["score"] for d in dt], "gtIgnore": gtIg,
            "dtIgnore": dtIg}


def _accumulate(eval_imgs, K, A, I, max_dets, with_scores):
    """COCOeval.accumulate (with_scores) / LVISEval.accumulate (max_dets = [None])."""
    T, R, M = len(_iou_thrs()), len(_rec_thrs()), len(max_dets)
    rec = _rec_thrs()
    precision = -np.ones((T, R, K, A, M))
    recall = -np.ones((T, K, A, M))
    scores = -np.ones((T, R, K, A, M))
    for k in range(K):
        Nk = k * A * I
        for a in range(A):
            Na = a * I
            for m, maxDet in enumerate(max_dets):
                E = [eval_imgs[Nk + Na + i] for i in range(I)]
                E = [e for e in E if e is not None]
                if len(E) == 0:
                    continue
                dtScores = np.concatenate([e["dtScores"][0:maxDet] for e in E])
                inds = np.argsort(-dtScores, kind="mergesort")
                dtScoresSorted = dtScores[inds]
                dtm = np.concatenate([e["dtMatches"][:, 0:maxDet] for e in E], axis=1)[:, inds]
                dtIg = np.concatenate([e["dtIgnore"][:, 0:maxDet] for e in E], axis=1)[:, inds]
                gtIg = np.concatenate([e["gtIgnore"] for e in E])
                npig = np.count_nonzero(gtIg == 0)
                if npig == 0:
                    continue
                tps = np.logical_and(dtm, np.logical_not(dtIg))
                fps = np.logical_and(np.logical_not(dtm), np.logical_not(dtIg))
                tp_sum = np.cumsum(tps, axis=1).astype(dtype=np.float64)
                fp_sum = np.cumsum(fps, axis=1).astype(dtype=np.float64)
                for t, (tp, fp) in enumerate(zip(tp_sum, fp_sum)):
                    tp = np.array(tp)
                    fp = np.array(fp)
                    nd = len(tp)
                    rc = tp / npig
                    pr = tp / (fp + tp + np.spacing(1))
                    q = np.zeros((R,))
                    ss = np.zeros((R,))
                    recall[t, k, a, m] = rc[-1] if nd else 0
                    pr = pr.tolist()
                    q = q.tolist()
                    for i in range(nd - 1, 0, -1):
                        if pr[i] > pr[i - 1]:
                            pr[i - 1] = pr[i]
                    inds = np.searchsorted(rc, rec, side="left")
                    try:
                        for ri, pi in enumerate(inds):
                            q[ri] = pr[pi]
                            ss[ri] = dtScoresSorted[pi]
                    except IndexError:
                        pass
                    precision[t, :, k, a, m] = np.array(q)
                    scores[t, :, k, a, m] = np.array(ss)
    return precision, recall, (scores if with_scores else None)


def _summ(s):
    return -1 if len(s[s > -1]) == 0 else np.mean(s[s > -1])


def coco_eval(ann, dets, max_dets=(100, 300, 1000)):
    """COCOeval(bbox) after CocoMetric: returns dict(precision, recall, scores, stats)."""
    max_dets = list(max_dets)
    img_ids = list(np.unique([im["id"] for im in ann["images"]]))
    cat_ids = list(np.unique([c["id"] for c in ann["categories"]]))
    si, sc = set(img_ids), set(cat_ids)
    gts = [dict(a) for a in ann["annotations"] if a["image_id"] in si and a["category_id"] in sc]
    dts = []
    for n, r in enumerate(results_list(dets)):              # loadRes: area, id, iscrowd
        r["area"] = r["bbox"][2] * r["bbox"][3]
        r["id"] = n + 1
        r["iscrowd"] = 0
        if r["image_id"] in si and r["category_id"] in sc:
            dts.append(r)
    for gt in gts:
        gt["ignore"] = gt["ignore"] if "ignore" in gt else 0
        gt["ignore"] = "iscrowd" in gt and gt["iscrowd"]
    _gts, _dts = defaultdict(list), defaultdict(list)
    for gt in gts:
        _gts[gt["image_id"], gt["category_id"]].append(gt)
    for dt in dts:
        _dts[dt["image_id"], dt["category_id"]].append(dt)
    thrs = _iou_thrs()
    ious = {}
    for i in img_ids:
        for c in cat_ids:
            gt, dt = _gts[i, c], _dts[i, c]
            if len(gt) == 0 and len(dt) == 0:
                ious[i, c] = []
                continue
            inds = np.argsort([-d["score"] for d in dt], kind="mergesort")
            dt = [dt[j] for j in inds][0:max_dets[-1]]
            ious[i, c] = _iou([d["bbox"] for d in dt], [g["bbox"] for g in gt], [int(o["iscrowd"]) for o in gt])
    eval_imgs = [_evaluate_img(_gts[i, c], _dts[i, c], ious[i, c], a, max_dets[-1], thrs, True)
                 for c in cat_ids for a in AREA_RNG for i in img_ids]
    precision, recall, scores = _accumulate(eval_imgs, len(cat_ids), len(AREA_RNG), len(img_ids), max_dets, True)

    def s(ap=1, iouThr=None, areaRng="all", maxDets=100):
        aind = [i for i, aRng in enumerate(AREA_LBL) if aRng == areaRng]
        mind = [i for i, mDet in enumerate(max_dets) if mDet == maxDets]
        x = precision if ap == 1 else recall
        if iouThr is not None:
            x = x[np.where(iouThr == thrs)[0]]
        x = x[:, :, :, aind, mind] if ap == 1 else x[:, :, aind, mind]
        return _summ(x)

    m0, m1, m2 = max_dets
    stats = np.array([s(1), s(1, .5, maxDets=m2), s(1, .75, maxDets=m2), s(1, areaRng="small", maxDets=m2),
                      s(1, areaRng="medium", maxDets=m2), s(1, areaRng="large", maxDets=m2), s(0, maxDets=m0),
                      s(0, maxDets=m1), s(0, maxDets=m2), s(0, areaRng="small", maxDets=m2),
                      s(0, areaRng="medium", maxDets=m2), s(0, areaRng="large", maxDets=m2)], np.float64)
    return dict(precision=precision, recall=recall, scores=scores, stats=stats)


def lvis_eval(ann, dets, max_dets=300):
    """LVISResults(max_dets) + LVISEval(bbox): returns dict(precision [T,R,K,A], recall [T,K,A], stats)."""
    result_anns = results_list(dets)
    img_ann = defaultdict(list)                               # LVISResults.limit_dets_per_image
    for a in result_anns:
        img_ann[a["image_id"]].append(a)
    for img_id, _anns in img_ann.items():
        if len(_anns) <= max_dets:
            continue
        img_ann[img_id] = sorted(_anns, key=lambda a: a["score"], reverse=True)[:max_dets]
    result_anns = [a for anns in img_ann.values() for a in anns]
    for n, a in enumerate(result_anns):
        a["area"] = a["bbox"][2] * a["bbox"][3]
        a["id"] = n + 1
    img_ids = sorted(im["id"] for im in ann["images"])
    img_ids = list(np.unique(img_ids))
    cats = sorted(ann["categories"], key=lambda c: c["id"])
    cat_ids = [c["id"] for c in cats]
    si, sc = set(img_ids), set(cat_ids)
    gts = [dict(a) for a in ann["annotations"] if a["image_id"] in si and a["category_id"] in sc]
    dts = [a for a in result_anns if a["image_id"] in si and a["category_id"] in sc]
    for gt in gts:
        if "ignore" not in gt:
            gt["ignore"] = 0
    _gts, _dts = defaultdict(list), defaultdict(list)
    for gt in gts:
        _gts[gt["image_id"], gt["category_id"]].append(gt)
    img_data = {im["id"]: im for im in ann["images"]}
    img_nl = {i: img_data[i].get("neg_category_ids", []) for i in img_ids}
    img_pl = defaultdict(set)
    for a in gts:
        img_pl[a["image_id"]].add(a["category_id"])
    img_nel = {i: img_data[i].get("not_exhaustive_category_ids", []) for i in img_ids}
    for dt in dts:
        i, c = dt["image_id"], dt["category_id"]
        if c not in img_nl[i] and c not in img_pl[i]:
            continue
        _dts[i, c].append(dt)
    freq_groups = [[] for _ in "rcf"]
    for idx, c in enumerate(cats):
        freq_groups["rcf".index(c["frequency"])].append(idx)
    thrs = _iou_thrs()
    ious = {}
    for i in img_ids:
        for c in cat_ids:
            gt, dt = _gts[i, c], _dts[i, c]
            if len(gt) == 0 and len(dt) == 0:
                ious[i, c] = []
                continue
            idx = np.argsort([-d["score"] for d in dt], kind="mergesort")
            dt = [dt[j] for j in idx]
            ious[i, c] = _iou([d["bbox"] for d in dt], [g["bbox"] for g in gt], [0] * len(gt))
    eval_imgs = [_evaluate_img(_gts[i, c], _dts[i, c], ious[i, c], a, None, thrs, False, img_nel)
                 for c in cat_ids for a in AREA_RNG for i in img_ids]
    precision, recall, _ = _accumulate(eval_imgs, len(cat_ids), len(AREA_RNG), len(img_ids), [None], False)
    precision, recall = precision[..., 0], recall[..., 0]

    def s(kind, iou_thr=None, area_rng="all", fg=None):
        aidx = [i for i, a in enumerate(AREA_LBL) if a == area_rng]
        x = precision if kind == "ap" else recall
        if iou_thr is not None:
            x = x[np.where(iou_thr == thrs)[0]]
        if kind == "ap":
            x = x[:, :, freq_groups[fg], aidx] if fg is not None else x[:, :, :, aidx]
        else:
            x = x[:, :, aidx]
        return _summ(x)

    stats = np.array([s("ap"), s("ap", .5), s("ap", .75), s("ap", area_rng="small"), s("ap", area_rng="medium"),
                      s("ap", area_rng="large"), s("ap", fg=0), s("ap", fg=1), s("ap", fg=2), s("ar"),
                      s("ar", area_rng="small"), s("ar", area_rng="medium"), s("ar", area_rng="large")], np.float64)
    return dict(precision=precision, recall=recall, stats=stats, freq_groups=freq_groups)


# ------------------------------------------------------------------------------------------ synthetic sets
def make_set(seed, n_img=40, n_cat=6, lvis=False, dets_per_img=30, gts_per_img=(0, 8), tie_levels=None,
             crowd_frac=0.1, empty_frac=0.1, no_det_frac=0.1, extra=None, fixed_dets=False):
    """Seeded COCO- or LVIS-format annotation dict plus per-image detections near the gts.  Image and category ids
    are shuffled and non-contiguous; some images are empty, some have gts and no dets, the last category has no gt;
    ``tie_levels`` quantises the scores (many ties); ``extra`` = list of (image index, category index, n_dets, n_gts)
    pairs to add (large pairs); ``fixed_dets``: exactly ``dets_per_img`` dets on every image that has dets."""
    rng = np.random.default_rng(seed)
    img_ids = rng.permutation(np.arange(1, 3 * n_img + 1))[:n_img] * 7 + 3
    cat_ids = rng.permutation(np.arange(1, 4 * n_cat + 1))[:n_cat] * 5 + 1
    images, anns, dets = [], [], []
    ann_id = 1

    def box(size):
        x, y = rng.uniform(0, 600, 2)
        w, h = rng.uniform(2, size, 2)
        return [float(x), float(y), float(w), float(h)]

    per_img = {}
    for n, i in enumerate(img_ids):
        im = dict(id=int(i), file_name=f"{int(i):012d}.jpg", width=640, height=640)
        kind = rng.random()
        gts = []
        if kind >= empty_frac:
            for _ in range(int(rng.integers(gts_per_img[0], gts_per_img[1] + 1))):
                c = int(cat_ids[rng.integers(0, n_cat - 1)])
                gts.append((c, box(rng.choice([20, 60, 200]))))
        for e in (extra or []):
            if e[0] == n:
                for _ in range(e[3]):
                    gts.append((int(cat_ids[e[1]]), box(120)))
        for c, b in gts:
            area = b[2] * b[3] * (1.0 if rng.random() < 0.7 else float(rng.uniform(0.3, 1.5)))
            a = dict(id=ann_id, image_id=int(i), category_id=c, bbox=b, area=area)
            if not lvis:
                a["iscrowd"] = int(rng.random() < crowd_frac)
            anns.append(a)
            ann_id += 1
        if lvis:
            present = {c for c, _ in gts}
            others = [int(c) for c in cat_ids if int(c) not in present]
            im["neg_category_ids"] = [c for c in others if rng.random() < 0.5]
            im["not_exhaustive_category_ids"] = [c for c in present if rng.random() < 0.3]
        images.append(im)
        per_img[n] = gts
    for n, i in enumerate(img_ids):
        if rng.random() < no_det_frac:
            continue
        gts = per_img[n]
        nd = dets_per_img if fixed_dets else int(rng.integers(0, dets_per_img + 1))
        bxs, scs, cts = [], [], []
        for _ in range(nd):
            if gts and rng.random() < 0.7:
                c, g = gts[int(rng.integers(0, len(gts)))]
                j = rng.normal(0, 0.08, 4) * np.array([g[2], g[3], g[2], g[3]])
                x1, y1 = g[0] + j[0], g[1] + j[1]
                x2, y2 = g[0] + g[2] + j[2], g[1] + g[3] + j[3]
                if rng.random() < 0.1:
                    c = int(cat_ids[rng.integers(0, n_cat)])
            else:
                c = int(cat_ids[rng.integers(0, n_cat)])
                b = box(150)
                x1, y1, x2, y2 = b[0], b[1], b[0] + b[2], b[1] + b[3]
            bxs.append([x1, y1, x2, y2])
            scs.append(rng.random())
            cts.append(c)
        for e in (extra or []):
            if e[0] == n:
                g = [gg for cc, gg in gts if cc == int(cat_ids[e[1]])]
                for q in range(e[2]):
                    b = g[q % len(g)] if g else box(120)
                    j = rng.normal(0, 0.1, 4) * 20
                    bxs.append([b[0] + j[0], b[1] + j[1], b[0] + b[2] + j[2], b[1] + b[3] + j[3]])
                    scs.append(rng.random())
                    cts.append(int(cat_ids[e[1]]))
        s = np.asarray(scs, np.float32)
        if tie_levels:
            s = (np.floor(s * tie_levels) / tie_levels).astype(np.float32)
        dets.append(dict(image_id=int(i), bboxes=np.asarray(bxs, np.float32).reshape(-1, 4), scores=s,
                         category_ids=np.asarray(cts, np.int64)))
    cats = [dict(id=int(c), name=f"cat{int(c)}") for c in cat_ids]
    if lvis:
        for k, c in enumerate(cats):
            c["frequency"] = "rcf"[k % 3]
    return dict(images=images, annotations=anns, categories=cats), dets
