"""numpy restatement of the reference's single-label branch, YOLOWorldHead.predict_by_feat with ``multi_label=False``
(yolo_world_head.py:712-746), built on the oracle's pieces:

    scores, labels = scores.max(1, keepdim=True)                                      (first occurrence on ties)
    scores, _, keep_idxs, results = filter_scores_and_topk(scores, score_thr, nms_pre, results=dict(labels=labels[:, 0]))
    bboxes = (bboxes[keep_idxs] - pad) / scale_factor                                  (rescale)
    mmdet _bbox_post_process: mmcv.ops.batched_nms(bboxes, scores, labels, cfg.nms)[:max_per_img], clamp

tests/golden/best_class.npz (tests/golden/make_golden_best.py) holds what the reference's own functions return for the first
two lines; tests/test_cpu_best.py holds this file against it."""
from __future__ import annotations

import numpy as np

from oracle import postprocess as opp

f32 = np.float32


def best_class(scores: np.ndarray):
    """[N, K] -> (best score [N] fp32, label [N] int64): ``Tensor.max(1)`` / ``numpy.argmax``, the lowest class on ties."""
    scores = np.ascontiguousarray(scores, dtype=f32)
    lab = np.argmax(scores, axis=1).astype(np.int64)
    return scores[np.arange(scores.shape[0]), lab], lab


def candidates(scores: np.ndarray, score_thr: float, nms_pre: int):
    """(scores [n], labels [n], anchors [n]) of one image: the best class per row through filter_scores_and_topk."""
    best, lab = best_class(scores)
    s, _, anchors = opp.filter_scores_and_topk(best[:, None], score_thr, nms_pre)
    return s, lab[anchors], anchors


def nms_rows(cand_boxes: np.ndarray, s: np.ndarray, labels: np.ndarray, meta, iou_thr: float, max_out: int, split_thr: int,
             class_agnostic: bool):
    """Candidates (sorted) -> kept rows, with the 8 floats of wd_nms_gather's per-image metadata: rescale before NMS when
    meta[7] != 0 (the mmdet order), after it otherwise; clamp last."""
    pad, scale, ori_hw, pre = (meta[0], meta[1]), (meta[3], meta[4]), (meta[6], meta[5]), meta[7] != 0
    b = np.ascontiguousarray(cand_boxes, dtype=f32)
    if b.shape[0] == 0:
        return dict(bboxes=np.zeros((0, 4), f32), keep=np.zeros(0, np.int64))
    if pre:
        b = opp.rescale_boxes(b, pad, scale)
    cfg = dict(type="nms", iou_threshold=iou_thr, split_thr=split_thr, class_agnostic=bool(class_agnostic))
    keep = opp.mmcv_batched_nms(b, s, labels, cfg, max_keep=max_out)
    out = b[keep] if pre else opp.rescale_boxes(b[keep], pad, scale)
    return dict(bboxes=opp.clamp_boxes(out, ori_hw), keep=keep)


def predict_image(boxes: np.ndarray, scores: np.ndarray, meta, score_thr: float, nms_pre: int, iou_thr: float, max_per_img: int,
                  split_thr: int = opp.MMCV_SPLIT_THR, class_agnostic: bool = False):
    """One image of predict_by_feat(multi_label=False): boxes [N, 4], scores [N, K] (the columns of its own bank only)."""
    s, labels, anchors = candidates(scores, score_thr, nms_pre)
    r = nms_rows(boxes[anchors], s, labels, meta, iou_thr, max_per_img, split_thr, class_agnostic)
    keep = r["keep"]
    return dict(bboxes=r["bboxes"], scores=s[keep], labels=labels[keep], anchors=anchors[keep])
