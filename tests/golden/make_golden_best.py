#!/usr/bin/env python3
"""Generate tests/golden/best_class.npz by IMPORTING the reference (like make_golden.py: only where the reference tree is
present; CPU).  The single-label branch of YOLOWorldHead.predict_by_feat (yolo_world_head.py:712-722) on seeded scores:

    scores, labels = scores.max(1, keepdim=True)
    scores, _, keep_idxs, results = filter_scores_and_topk(scores, score_thr, nms_pre, results=dict(labels=labels[:, 0]))

with the reference's own ``filter_scores_and_topk`` (generate_proposal.py:85-131, the twin of mmdet's), its sort forced stable
(SURVEY.md §7).  Inputs: 2 images x 525 anchors x 300 classes, scores on a 4096-level grid (so that equal scores occur by
themselves) with planted exact ties: a row whose maximum sits in classes 7 and 150 and 299, a row that is constant, two rows
with the same maximum (the top-k tie, broken by the anchor), the maximum in class 0 and in class 299.  Only data is written.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_best.py
"""
import sys
sys.dont_write_bytecode = True

import os

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import make_golden as MG                       # noqa: E402  (import_generate_proposal, stable_sort)

B, N, K = 2, 525, 300
SCORE_THR, NMS_PRE = 0.995, 400


def levels_to_scores(q: np.ndarray) -> np.ndarray:
    """uint16 levels -> fp32 scores in (0, 1]: (q + 1) / 4096, exact."""
    return ((q.astype(np.float32) + np.float32(1)) / np.float32(4096)).astype(np.float32)


def main():
    gp = MG.import_generate_proposal()
    g = np.random.default_rng(20250)
    q = g.integers(0, 4096, (B, N, K)).astype(np.uint16)
    q[0, 10, :] = np.minimum(q[0, 10, :], 4000); q[0, 10, [7, 150, 299]] = 4090          # three classes tie: label 7
    q[0, 11, :] = 4085                                                                    # a constant row: label 0
    q[0, 200, :] = np.minimum(q[0, 200, :], 4000); q[0, 200, 0] = 4093                    # the maximum in class 0
    q[0, 201, :] = np.minimum(q[0, 201, :], 4000); q[0, 201, 299] = 4093                  # ... and in the last class, same score
    q[1, 3, :] = np.minimum(q[1, 3, :], 4000); q[1, 3, [298, 299]] = 4095
    q[1, 524, :] = np.minimum(q[1, 524, :], 4000); q[1, 524, 1] = 4095                    # ties with row 3 in the top-k
    fx = {"levels": q, "score_thr": np.float32(SCORE_THR), "nms_pre": np.int64(NMS_PRE)}
    for b in range(B):
        sc = torch.from_numpy(levels_to_scores(q[b]))
        with MG.stable_sort():
            s, labels = sc.max(1, keepdim=True)
            s, _, keep_idxs, results = gp.filter_scores_and_topk(s, SCORE_THR, NMS_PRE, results=dict(labels=labels[:, 0]))
        fx[f"img{b}.scores"] = s.numpy()
        fx[f"img{b}.labels"] = results["labels"].numpy().astype(np.int64)
        fx[f"img{b}.anchors"] = keep_idxs.numpy().astype(np.int64)
        print(f"img{b}: {s.shape[0]} candidates, {int((np.diff(s.numpy()) == 0).sum())} equal neighbours")
    out = os.path.join(HERE, "best_class.npz")
    np.savez_compressed(out, **fx)
    print("wrote", out, os.path.getsize(out), "bytes")


if __name__ == "__main__":
    main()
