"""COCO and LVIS box mAP with the matching and accumulation on the device (``wd_det_match`` / ``wd_det_sort`` /
``wd_det_accumulate``, csrc/det_eval.hip).

    ev = coco_evaluate(ann, dets)            # ann: the parsed instances JSON; dets: per image dict(image_id,
    ev = lvis_evaluate(ann, dets)            #   bboxes [n, 4] xyxy fp32, scores [n] fp32, category_ids [n])
    ev["precision"], ev["recall"], ev["scores"], ev["stats"], ev["metrics"], ev.get("classwise")

The result equals what pycocotools 2.x (``COCOeval`` bbox, ``maskApi.c``) and lvis-api (``LVISEval`` / ``LVISResults``)
compute from the same detections after mmdet 3.3's ``CocoMetric`` / ``LVISMetric`` wrote them as a results file.
Neither library is needed: the rules are restated here, loop for loop in tests/det_eval_ref.py, and the device arrays
are compared with that restatement by ``np.array_equal``.

Rules (both metrics)
  * A det box is ``[x1, y1, float(x2) - float(x1), float(y2) - float(y1)]`` in float64 from the fp32 outputs (mmdet
    ``xyxy2xywh`` after ``.tolist()``); its area is ``w * h`` (``loadRes`` / ``LVISResults``).  Scores are the fp32
    values as float64.
  * IoU is ``bbIou``: ``w = fmin(D[0]+D[2], G[0]+G[2]) - fmax(D[0], G[0])``, likewise ``h``; ``w <= 0`` or ``h <= 0``
    gives 0; else ``i = w * h`` over ``da + ga - i``, or over ``da`` when the gt is crowd.  ``da`` / ``ga`` are box
    ``w * h``, not the JSON ``area``.  No fused multiply-add anywhere.
  * Image ids and category ids are ``np.unique``-sorted (all images and categories of the annotation file).  Dets
    whose image or category is not among them are dropped.  Gts and dets of an (image, category) pair keep the
    order of the annotation file / the results.
  * Area ranges ``[0, 1e10], [0, 32^2], [32^2, 96^2], [96^2, 1e10]`` (all, small, medium, large); a gt is area-ignored
    when its JSON ``area`` is outside the range.  ``iouThrs = linspace(.5, .95, 10)``, ``recThrs = linspace(0, 1,
    101)``, built as the libraries build them; a match needs ``IoU >= min(t, 1 - 1e-10)``.
  * Per pair the dets are sorted by score, descending and stable; the gts by area-ignore flag, stable, per range.
    Greedy matching per (threshold, range): each det, in order, takes the unmatched (or crowd) gt of largest IoU
    reaching the threshold, a later gt on ties winning; once it holds a kept gt it stops at the first ignored one.
    A det matched to an ignored gt is ignored; an unmatched det outside the area range is ignored.  A match with a
    gt whose ``id`` is 0 counts as unmatched (the libraries store the matched id and test it for nonzero).
  * accumulate: per (category, range, maxDet) the dets of all pairs with rank below maxDet, ordered by score
    descending, then image position, then rank (numpy's mergesort on the concatenation); integer prefix sums of TP
    and FP; ``rc = tp / npig``, ``pr = tp / (fp + tp + 2^-52)``; the reverse running max of ``pr``; left-side
    ``searchsorted`` of the recall thresholds, and every threshold past the last recall stays 0 (the libraries'
    caught IndexError).  ``scores`` holds the sorted score at the same index.  A (category, range) without a kept gt
    stays -1 everywhere.  ``recall = rc[-1]``, or 0 without dets.
  * The stats are the libraries' ``summarize``: means over the entries > -1 of the selected slices, -1 if none.

COCO only
  * The gt ``ignore`` flag is its ``iscrowd`` (this replaces any ``ignore`` field); crowd gts use the crowd IoU and
    may be matched again.
  * ``maxDets = [100, 300, 1000]`` (mmdet's ``proposal_nums`` replace pycocotools' default); truncation at 1000 per
    pair happens before matching.
  * 12 stats (``_summarizeDets``): AP at maxDets 100 (``_summarize(1)`` keeps its default of 100, so mmdet's
    ``bbox_mAP`` is AP@100), AP50, AP75, AP s/m/l at 1000, AR@100, AR@300, AR@1000, AR s/m/l at 1000; mmdet's names
    ``bbox_mAP``, ``bbox_mAP_50``, ``bbox_mAP_75``, ``bbox_mAP_s/m/l``, ``bbox_mAP_copypaste``, rounded to 3 places.

LVIS only
  * First the 300 highest-scoring dets per image across all categories (stable, ``LVISResults(max_dets=300)``).
  * A det is kept only if its category is among the image's gt categories or its ``neg_category_ids``.
  * No crowd: the gt ``ignore`` field counts when present (0 otherwise); ``iscrowd`` is not read.
  * An unmatched det whose category is in the image's ``not_exhaustive_category_ids`` is ignored.
  * No per-pair truncation; ``precision`` is ``[T, R, K, A]``, ``recall`` ``[T, K, A]`` (no ``scores``).
  * 13 stats: AP, AP50, AP75, APs, APm, APl, APr, APc, APf (categories grouped by their ``frequency`` r / c / f),
    AR@300 and ARs/ARm/ARl@300; mmdet's names ``bbox_AP`` ... ``bbox_APf``.

Building the pair layout from the flat arrays is numpy; ranking, IoU, matching, sorting and accumulation run on the
device.  The per-class table (``classwise=True``) is mmdet's: per category the mean of ``precision[:, :, k, 0, -1]``
over entries > -1 (``nan`` when there are none).
"""
from __future__ import annotations

from typing import Dict, List, Optional, Sequence

import numpy as np
import torch

from . import lib as L

AREA_RNG = [[0 ** 2, 1e5 ** 2], [0 ** 2, 32 ** 2], [32 ** 2, 96 ** 2], [96 ** 2, 1e5 ** 2]]
AREA_LBL = ["all", "small", "medium", "large"]
COCO_MAX_DETS = [100, 300, 1000]
LVIS_MAX_DETS = 300
COCO_METRIC_NAMES = ["mAP", "mAP_50", "mAP_75", "mAP_s", "mAP_m", "mAP_l",
                     "AR@100", "AR@300", "AR@1000", "AR_s@1000", "AR_m@1000", "AR_l@1000"]
LVIS_METRIC_NAMES = ["AP", "AP50", "AP75", "APs", "APm", "APl", "APr", "APc", "APf"]
LVIS_STAT_NAMES = LVIS_METRIC_NAMES + ["AR@300", "ARs@300", "ARm@300", "ARl@300"]

_GT_IGNORE, _GT_CROWD, _GT_ID_NONZERO = 1, 2, 4


def iou_thrs() -> np.ndarray:
    return np.linspace(.5, 0.95, int(np.round((0.95 - .5) / .05)) + 1, endpoint=True)


def rec_thrs() -> np.ndarray:
    return np.linspace(.0, 1.00, int(np.round((1.00 - .0) / .01)) + 1, endpoint=True)


# ------------------------------------------------------------------------------------------ input flattening
def flatten_dets(dets: Sequence[dict]):
    """Per-image dicts -> flat arrays in results order: image ids, category ids, xyxy fp32 boxes, fp32 scores."""
    img, cat, box, score = [], [], [], []
    for d in dets:
        b = np.asarray(d["bboxes"], np.float32).reshape(-1, 4)
        s = np.asarray(d["scores"], np.float32).reshape(-1)
        c = np.asarray(d["category_ids"], np.int64).reshape(-1)
        if not (b.shape[0] == s.shape[0] == c.shape[0]):
            raise ValueError(f"image {d.get('image_id')}: bboxes, scores and category_ids differ in length")
        img.append(np.full(s.shape[0], int(d["image_id"]), np.int64))
        cat.append(c)
        box.append(b)
        score.append(s)
    if not img:
        return np.zeros(0, np.int64), np.zeros(0, np.int64), np.zeros((0, 4), np.float32), np.zeros(0, np.float32)
    return np.concatenate(img), np.concatenate(cat), np.concatenate(box), np.concatenate(score)


def _gt_arrays(ann: dict, lvis: bool):
    anns = ann.get("annotations", [])
    n = len(anns)
    img = np.fromiter((a["image_id"] for a in anns), np.int64, n)
    cat = np.fromiter((a["category_id"] for a in anns), np.int64, n)
    box = np.asarray([a["bbox"] for a in anns], np.float64).reshape(n, 4)
    area = np.fromiter((a["area"] for a in anns), np.float64, n)
    if lvis:
        ign = np.fromiter((bool(a.get("ignore", 0)) for a in anns), bool, n)
        crowd = np.zeros(n, bool)
    else:
        crowd = np.fromiter((bool(a.get("iscrowd", 0)) for a in anns), bool, n)
        ign = crowd
    idnz = np.fromiter((a["id"] != 0 for a in anns), bool, n)
    flag = (ign * _GT_IGNORE | crowd * _GT_CROWD | idnz * _GT_ID_NONZERO).astype(np.uint8)
    return img, cat, box, area, flag


# ------------------------------------------------------------------------------------------ device evaluation
def _device_eval(img_ids, cat_ids, gt, dt, max_dets: List[int], trunc: int, with_scores: bool, device):
    """gt = (img, cat, box xywh f64, area f64, flag u8), dt = (img, cat, box xyxy f32, score f32, flag u8), already
    restricted to img_ids x cat_ids -> precision [T, R, K, A, M], recall [T, K, A, M], scores or None."""
    T, R, K, A, M = 10, 101, len(cat_ids), 4, len(max_dets)
    n_img = len(img_ids)
    gkey = np.searchsorted(cat_ids, gt[1]) * n_img + np.searchsorted(img_ids, gt[0])
    dkey = np.searchsorted(cat_ids, dt[1]) * n_img + np.searchsorted(img_ids, dt[0])
    go = np.argsort(gkey, kind="stable")
    do = np.argsort(dkey, kind="stable")
    gk, dk = gkey[go], dkey[do]
    pkeys = np.union1d(gk, dk)
    P = pkeys.shape[0]
    g_off = np.searchsorted(gk, pkeys, "left").astype(np.int64)
    d_off = np.searchsorted(dk, pkeys, "left").astype(np.int64)
    g_off = np.append(g_off, gk.shape[0])
    d_off = np.append(d_off, dk.shape[0])
    n_det = np.diff(d_off)
    n_gt = np.diff(g_off)
    kept = np.minimum(n_det, trunc)
    slot_off = np.zeros(P + 1, np.int64)
    slot_off[1:] = np.cumsum(kept)
    n_slot = int(slot_off[-1])
    if n_slot >= 2 ** 31 - 1 or dk.shape[0] >= 2 ** 31 - 1 or gk.shape[0] >= 2 ** 31 - 1:
        raise L.WedetectHipError("det_eval handles fewer than 2^31 dets / gts")
    pair_cat = (pkeys // max(n_img, 1)).astype(np.int32)
    cat_pair_off = np.searchsorted(pair_cat, np.arange(K + 1)).astype(np.int64)
    cat_slot_off = slot_off[cat_pair_off]
    # per-pair workspace (csrc/det_eval.hip match_workspace_bytes); pairs above the LDS slice get a scratch slice
    need = 8 * kept * n_gt + 4 * kept + 4 * 40 * ((n_gt + 31) // 32) + n_gt
    need = (need + 15) & ~15
    big = need > int(L.LIB.wd_det_match_lds_bytes())
    scr = np.full(P, -1, np.int64)
    scr[big] = np.concatenate([[0], np.cumsum(need[big])[:-1]]) if big.any() else np.zeros(0, np.int64)
    scr_bytes = int(need[big].sum()) if big.any() else 16

    dev = torch.device(device)
    i32 = lambda a: torch.from_numpy(np.ascontiguousarray(a, np.int32)).to(dev)
    f64 = lambda a: torch.from_numpy(np.ascontiguousarray(a, np.float64)).to(dev)
    nz = lambda a, shape, dt: torch.from_numpy(np.ascontiguousarray(a, dt)).to(dev) if a.shape[0] else torch.zeros(shape, dtype=getattr(torch, np.dtype(dt).name), device=dev)
    t_pair_det, t_pair_gt, t_slot = i32(d_off), i32(g_off), i32(slot_off)
    t_pcat = i32(pair_cat) if P else torch.zeros(1, dtype=torch.int32, device=dev)
    t_scr_off = torch.from_numpy(scr).to(dev) if P else torch.zeros(1, dtype=torch.int64, device=dev)
    t_dbox = nz(dt[2][do], (1, 4), np.float32)
    t_dscore = nz(dt[3][do], (1,), np.float32)
    t_dflag = nz(dt[4][do], (1,), np.uint8)
    t_gbox = nz(gt[2][go], (1, 4), np.float64)
    t_garea = nz(gt[3][go], (1,), np.float64)
    t_gflag = nz(gt[4][go], (1,), np.uint8)
    thr = f64([min(t, 1 - 1e-10) for t in iou_thrs()])
    rng = f64(np.asarray(AREA_RNG, np.float64).reshape(-1))
    scratch = torch.empty(scr_bytes, dtype=torch.uint8, device=dev)
    ns = max(n_slot, 1)
    n2 = 2
    while n2 < ns:
        n2 *= 2
    slot_score = torch.empty(ns, dtype=torch.float32, device=dev)
    slot_rank = torch.empty(ns, dtype=torch.int32, device=dev)
    sort_keys = torch.full((n2, 2), -1, dtype=torch.int64, device=dev)    # WdDetSortKey {key, val, pad}: padding = ones
    flags = torch.empty(40 * ns, dtype=torch.uint8, device=dev)
    npig = torch.zeros(max(P, 1) * 4, dtype=torch.int32, device=dev)
    err = torch.zeros(1, dtype=torch.int32, device=dev)
    L.check(L.LIB.wd_det_match(t_pair_det.data_ptr(), t_pair_gt.data_ptr(), t_slot.data_ptr(), t_pcat.data_ptr(),
                               t_scr_off.data_ptr(), P, t_dbox.data_ptr(), t_dscore.data_ptr(), t_dflag.data_ptr(),
                               t_gbox.data_ptr(), t_garea.data_ptr(), t_gflag.data_ptr(), thr.data_ptr(), rng.data_ptr(),
                               int(trunc), scratch.data_ptr(), slot_score.data_ptr(), slot_rank.data_ptr(),
                               sort_keys.data_ptr(), flags.data_ptr(), n_slot, npig.data_ptr(),
                               err.data_ptr(), L.stream_ptr()), "wd_det_match")
    if n_slot > 1:
        L.check(L.LIB.wd_det_sort(sort_keys.data_ptr(), n2, L.stream_ptr()), "wd_det_sort")
    precision = torch.full((T, R, K, A, M), -1.0, dtype=torch.float64, device=dev)
    recall = torch.full((T, K, A, M), -1.0, dtype=torch.float64, device=dev)
    scores = torch.full((T, R, K, A, M), -1.0, dtype=torch.float64, device=dev) if with_scores else None
    s_rank = torch.empty(ns, dtype=torch.int32, device=dev)
    s_score = torch.empty(ns, dtype=torch.float32, device=dev)
    s_flags = torch.empty(40 * ns, dtype=torch.uint8, device=dev)
    t_cat_slot, t_cat_pair, t_md, t_rec = i32(cat_slot_off), i32(cat_pair_off), i32(max_dets), f64(rec_thrs())
    L.check(L.LIB.wd_det_accumulate(sort_keys.data_ptr(), n_slot, slot_rank.data_ptr(), slot_score.data_ptr(),
                                    flags.data_ptr(), s_rank.data_ptr(), s_score.data_ptr(), s_flags.data_ptr(),
                                    t_cat_slot.data_ptr(), t_cat_pair.data_ptr(), npig.data_ptr(), K, t_rec.data_ptr(),
                                    t_md.data_ptr(), M, precision.data_ptr(), recall.data_ptr(),
                                    0 if scores is None else scores.data_ptr(), L.stream_ptr()), "wd_det_accumulate")
    if int(err.item()) != 0:
        raise L.WedetectHipError(f"wd_det_match rejected the pair layout (error bits {int(err.item())})")
    return (precision.cpu().numpy(), recall.cpu().numpy(), None if scores is None else scores.cpu().numpy())


# ------------------------------------------------------------------------------------------ summarize (numpy)
def _mean_valid(s: np.ndarray) -> float:
    return -1.0 if len(s[s > -1]) == 0 else float(np.mean(s[s > -1]))


def coco_summarize(precision, recall, max_dets=COCO_MAX_DETS) -> np.ndarray:
    """COCOeval.summarize (bbox) on eval arrays [T, R, K, A, M] / [T, K, A, M]."""
    thrs = iou_thrs()

    def _s(ap, iou_thr=None, area="all", md=100):
        aind = [i for i, a in enumerate(AREA_LBL) if a == area]
        mind = [i for i, m in enumerate(max_dets) if m == md]
        if ap == 1:
            s = precision
            if iou_thr is not None:
                s = s[np.where(iou_thr == thrs)[0]]
            s = s[:, :, :, aind, mind]
        else:
            s = recall
            if iou_thr is not None:
                s = s[np.where(iou_thr == thrs)[0]]
            s = s[:, :, aind, mind]
        return _mean_valid(s)

    m0, m1, m2 = max_dets
    return np.array([_s(1), _s(1, .5, md=m2), _s(1, .75, md=m2), _s(1, area="small", md=m2),
                     _s(1, area="medium", md=m2), _s(1, area="large", md=m2), _s(0, md=m0), _s(0, md=m1),
                     _s(0, md=m2), _s(0, area="small", md=m2), _s(0, area="medium", md=m2),
                     _s(0, area="large", md=m2)], np.float64)


def lvis_summarize(precision, recall, freq_groups) -> np.ndarray:
    """LVISEval.summarize on precision [T, R, K, A], recall [T, K, A]; freq_groups: category indices of r, c, f."""
    thrs = iou_thrs()

    def _s(kind, iou_thr=None, area="all", fg=None):
        aidx = [i for i, a in enumerate(AREA_LBL) if a == area]
        if kind == "ap":
            s = precision
            if iou_thr is not None:
                s = s[np.where(iou_thr == thrs)[0]]
            s = s[:, :, freq_groups[fg], aidx] if fg is not None else s[:, :, :, aidx]
        else:
            s = recall
            if iou_thr is not None:
                s = s[np.where(iou_thr == thrs)[0]]
            s = s[:, :, aidx]
        return _mean_valid(s)

    return np.array([_s("ap"), _s("ap", .5), _s("ap", .75), _s("ap", area="small"), _s("ap", area="medium"),
                     _s("ap", area="large"), _s("ap", fg=0), _s("ap", fg=1), _s("ap", fg=2), _s("ar"),
                     _s("ar", area="small"), _s("ar", area="medium"), _s("ar", area="large")], np.float64)


def _classwise(precision5: np.ndarray, names: List[str]) -> List[tuple]:
    """mmdet CocoMetric / LVISMetric per-class table: mean of precision[:, :, k, 0, -1] over entries > -1."""
    out = []
    for k, name in enumerate(names):
        p = precision5[:, :, k, 0, -1]
        p = p[p > -1]
        out.append((name, float(np.mean(p)) if p.size else float("nan")))
    return out


def _r3(v: float) -> float:
    return float(f"{round(float(v), 3)}")


# ------------------------------------------------------------------------------------------ public entry points
def coco_evaluate(ann: dict, dets: Sequence[dict], classwise: bool = False, device="cuda") -> Dict:
    """COCO box mAP (rules: module docstring).  ``dets``: per image ``dict(image_id, bboxes, scores,
    category_ids)``.  Returns ``precision`` [10, 101, K, 4, 3], ``recall`` [10, K, 4, 3], ``scores``, ``stats`` (12,
    float64), ``metrics`` (mmdet's names, 3 places) and with ``classwise`` a list of (category name, AP)."""
    img_ids = np.unique(np.asarray([im["id"] for im in ann.get("images", [])], np.int64))
    cats = sorted(ann.get("categories", []), key=lambda c: c["id"])
    cat_ids = np.unique(np.asarray([c["id"] for c in cats], np.int64))
    g_img, g_cat, g_box, g_area, g_flag = _gt_arrays(ann, lvis=False)
    gsel = np.isin(g_img, img_ids) & np.isin(g_cat, cat_ids)
    d_img, d_cat, d_box, d_score = flatten_dets(dets)
    dsel = np.isin(d_img, img_ids) & np.isin(d_cat, cat_ids)
    gt = (g_img[gsel], g_cat[gsel], g_box[gsel], g_area[gsel], g_flag[gsel])
    dt = (d_img[dsel], d_cat[dsel], d_box[dsel], d_score[dsel], np.zeros(int(dsel.sum()), np.uint8))
    precision, recall, scores = _device_eval(img_ids, cat_ids, gt, dt, COCO_MAX_DETS, COCO_MAX_DETS[-1], True, device)
    stats = coco_summarize(precision, recall)
    metrics = {f"bbox_{n}": _r3(v) for n, v in zip(COCO_METRIC_NAMES[:6], stats[:6])}
    metrics["bbox_mAP_copypaste"] = " ".join(f"{v:.3f}" for v in stats[:6])
    out = dict(precision=precision, recall=recall, scores=scores, stats=stats, metrics=metrics,
               img_ids=img_ids, cat_ids=cat_ids)
    if classwise:
        out["classwise"] = _classwise(precision, [c.get("name", str(c["id"])) for c in cats])
    return out


def lvis_keep(ann: dict, d_img, d_cat, d_score, max_dets: int = LVIS_MAX_DETS):
    """Boolean mask over flat dets: LVISResults' top-``max_dets`` per image (stable by score) and then LVISEval's
    federated filter (category among the image's gt categories or its ``neg_category_ids``)."""
    n = d_img.shape[0]
    order = np.lexsort((np.arange(n), -d_score.astype(np.float64), d_img))
    si = d_img[order]
    start = np.searchsorted(si, si, "left")
    top = np.zeros(n, bool)
    top[order] = (np.arange(n) - start) < max_dets
    img_ids = np.asarray([im["id"] for im in ann.get("images", [])], np.int64)
    cat_ids = np.asarray([c["id"] for c in ann.get("categories", [])], np.int64)
    ncat = int(cat_ids.max()) + 1 if cat_ids.size else 1
    pos = {int(a["image_id"]) * ncat + int(a["category_id"]) for a in ann.get("annotations", [])
           if a["category_id"] < ncat}
    neg = {int(im["id"]) * ncat + int(c) for im in ann.get("images", []) for c in im.get("neg_category_ids", [])
           if c < ncat}
    key = d_img * ncat + d_cat
    allowed = np.isin(key, np.fromiter(pos | neg, np.int64)) & np.isin(d_img, img_ids) & np.isin(d_cat, cat_ids)
    return top & allowed


def lvis_evaluate(ann: dict, dets: Sequence[dict], classwise: bool = False, device="cuda") -> Dict:
    """LVIS box mAP (rules: module docstring).  Returns ``precision`` [10, 101, K, 4], ``recall`` [10, K, 4],
    ``stats`` (13, float64), ``metrics`` (mmdet's names, 3 places), ``results`` (the 13 stats by lvis-api name) and
    with ``classwise`` a list of (category name, AP)."""
    img_ids = np.unique(np.asarray([im["id"] for im in ann.get("images", [])], np.int64))
    cats = sorted(ann.get("categories", []), key=lambda c: c["id"])
    cat_ids = np.unique(np.asarray([c["id"] for c in cats], np.int64))
    g_img, g_cat, g_box, g_area, g_flag = _gt_arrays(ann, lvis=True)
    gsel = np.isin(g_img, img_ids) & np.isin(g_cat, cat_ids)
    d_img, d_cat, d_box, d_score = flatten_dets(dets)
    dsel = lvis_keep(ann, d_img, d_cat, d_score)
    ncat = int(cat_ids.max()) + 1 if cat_ids.size else 1
    nel = {int(im["id"]) * ncat + int(c) for im in ann.get("images", [])
           for c in im.get("not_exhaustive_category_ids", []) if c < ncat}
    d_nel = np.isin(d_img * ncat + d_cat, np.fromiter(nel, np.int64)).astype(np.uint8)
    gt = (g_img[gsel], g_cat[gsel], g_box[gsel], g_area[gsel], g_flag[gsel])
    dt = (d_img[dsel], d_cat[dsel], d_box[dsel], d_score[dsel], d_nel[dsel])
    big = 2 ** 31 - 1
    precision, recall, _ = _device_eval(img_ids, cat_ids, gt, dt, [big], big, False, device)
    precision, recall = precision[..., 0], recall[..., 0]
    lbl = ["r", "c", "f"]
    freq_groups = [[] for _ in lbl]
    for k, c in enumerate(cats):
        freq_groups[lbl.index(c["frequency"])].append(k)
    stats = lvis_summarize(precision, recall, freq_groups)
    metrics = {f"bbox_{n}": _r3(v) for n, v in zip(LVIS_METRIC_NAMES, stats[:9])}
    out = dict(precision=precision, recall=recall, stats=stats, metrics=metrics,
               results=dict(zip(LVIS_STAT_NAMES, stats.tolist())), img_ids=img_ids, cat_ids=cat_ids)
    if classwise:
        out["classwise"] = _classwise(precision[..., None], [c.get("name", str(c["id"])) for c in cats])
    return out
