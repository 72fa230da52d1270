"""Exemplar prompts in numpy: the result definition of include/wedetect_hip_exemplar.h restated — example boxes to network
pixels, the fp32 IoU in the operation order of ``oracle.postprocess._iou_f32``, the first ``m`` candidates by (IoU descending,
anchor ascending), the class prototypes.  ``assign`` is vectorised; ``assign_loop`` is the brute-force loop it is tested against."""
from __future__ import annotations

import numpy as np

from oracle.postprocess import _iou_f32

f32 = np.float32


def to_network(box, meta_row) -> np.ndarray:
    """x' = x * scale_x + pad_x, y' = y * scale_y + pad_y: one fp32 multiply, then one fp32 add (numpy never fuses)."""
    box, mt = np.asarray(box, f32), np.asarray(meta_row, f32)
    scale, pad = np.array([mt[3], mt[4], mt[3], mt[4]], f32), np.array([mt[0], mt[1], mt[0], mt[1]], f32)
    return ((box * scale).astype(f32) + pad).astype(f32)


def pack_key(iou: np.ndarray, anchor: np.ndarray) -> np.ndarray:
    """(uint64) bits(iou) << 32 | (0xFFFFFFFF - anchor): larger is better."""
    return (np.asarray(iou, f32).view(np.uint32).astype(np.uint64) << np.uint64(32)) | (np.uint64(0xFFFFFFFF) - np.asarray(anchor).astype(np.uint64))


def assign(boxes, ex_boxes, ex_count, meta, m: int, min_iou: float):
    """boxes fp32 [B, N, 4] (network pixels), ex_boxes fp32 [B, max_ex, 4] (original pixels), ex_count int [B], meta fp32 [B, 8]
    -> sel_anchors int32 [B, max_ex * m], sel_iou fp32 [B, max_ex * m], sel_count int32 [B]."""
    boxes, ex_boxes, meta = np.asarray(boxes, f32), np.asarray(ex_boxes, f32), np.asarray(meta, f32)
    B, N, _ = boxes.shape
    max_ex = ex_boxes.shape[1]
    sel_a = np.full((B, max_ex * m), -1, np.int32)
    sel_i = np.zeros((B, max_ex * m), f32)
    sel_c = np.zeros(B, np.int32)
    thr = f32(min_iou)
    for b in range(B):
        cnt = min(max(int(ex_count[b]), 0), max_ex)
        sel_c[b] = cnt * m
        for e in range(cnt):
            with np.errstate(invalid="ignore", over="ignore"):
                iou = _iou_f32(to_network(ex_boxes[b, e], meta[b]), boxes[b]).astype(f32)
                cand = np.nonzero(iou > thr)[0]                # a NaN fails the comparison
            if cand.size == 0:
                continue
            key = pack_key(iou[cand], cand)                    # candidates have iou > 0: keys order like (iou desc, anchor asc)
            top = cand[np.argsort(key)[::-1][:m]]
            sel_a[b, e * m:e * m + top.size] = top
            sel_i[b, e * m:e * m + top.size] = iou[top]
    return sel_a, sel_i, sel_c


def assign_loop(boxes, ex_boxes, ex_count, meta, m: int, min_iou: float):
    """The same, one scalar fp32 operation at a time and a stable sort on (-iou, anchor)."""
    boxes, ex_boxes, meta = np.asarray(boxes, f32), np.asarray(ex_boxes, f32), np.asarray(meta, f32)
    B, N, _ = boxes.shape
    max_ex = ex_boxes.shape[1]
    sel_a = np.full((B, max_ex * m), -1, np.int32)
    sel_i = np.zeros((B, max_ex * m), f32)
    sel_c = np.zeros(B, np.int32)
    for b in range(B):
        cnt = min(max(int(ex_count[b]), 0), max_ex)
        sel_c[b] = cnt * m
        px, py, sx, sy = meta[b, 0], meta[b, 1], meta[b, 3], meta[b, 4]
        for e in range(cnt):
            x1, y1, x2, y2 = ex_boxes[b, e]
            x1, y1, x2, y2 = f32(f32(x1 * sx) + px), f32(f32(y1 * sy) + py), f32(f32(x2 * sx) + px), f32(f32(y2 * sy) + py)
            area_e = f32(f32(x2 - x1) * f32(y2 - y1))
            cands = []
            for n in range(N):
                a1, b1, a2, b2 = boxes[b, n]
                with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
                    area_n = f32(f32(a2 - a1) * f32(b2 - b1))
                    w = max(f32(0), f32(min(x2, a2) - max(x1, a1)))
                    h = max(f32(0), f32(min(y2, b2) - max(y1, b1)))
                    inter = f32(w * h)
                    iou = f32(inter / f32(f32(area_e + area_n) - inter))
                if iou > f32(min_iou):
                    cands.append((-float(iou), n, iou))
            cands.sort(key=lambda t: (t[0], t[1]))
            for j, (_, n, iou) in enumerate(cands[:m]):
                sel_a[b, e * m + j], sel_i[b, e * m + j] = n, iou
    return sel_a, sel_i, sel_c


def level_of(anchor, off1: int, off2: int):
    return (np.asarray(anchor) >= off1).astype(np.int64) + (np.asarray(anchor) >= off2).astype(np.int64)


def pool(level_embed, off1: int, off2: int, sel_anchors, sel_iou, cls_off, cls_slot):
    """The class prototypes in float64: level_embed [3, n_slot, dim], sel_anchors / sel_iou flat [n_slot], the CSR pair
    -> bank float64 [C, dim], support int32 [C], rows summed per class (= support)."""
    level_embed = np.asarray(level_embed, np.float64)
    sel_anchors, sel_iou = np.asarray(sel_anchors).reshape(-1), np.asarray(sel_iou, np.float64).reshape(-1)
    n_slot, dim = level_embed.shape[1:]
    C = len(cls_off) - 1
    bank, support = np.zeros((C, dim), np.float64), np.zeros(C, np.int32)
    for c in range(C):
        acc = np.zeros(dim, np.float64)
        for i in range(int(cls_off[c]), int(cls_off[c + 1])):
            s = int(cls_slot[i])
            if not 0 <= s < n_slot or sel_anchors[s] < 0:
                continue
            r = level_embed[int(level_of(sel_anchors[s], off1, off2)), s]
            with np.errstate(divide="ignore", invalid="ignore"):
                acc = acc + sel_iou[s] * (r * (1.0 / np.sqrt((r * r).sum())))
            support[c] += 1
        nrm = np.sqrt((acc * acc).sum())
        if support[c] > 0 and np.isfinite(nrm) and nrm > 0:
            bank[c] = acc / nrm
    return bank, support


def pool_bound(rows_summed: int) -> float:
    """|kernel - float64| per element: sequential fp32 summation of ``rows_summed`` terms bounded by 1, plus the two normalisations."""
    return (rows_summed + 8) * 2.0 ** -23
