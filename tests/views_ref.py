"""Numpy restatement of the test-time-augmentation path (include/wedetect_hip_views.h): the flip by ``np.flip``, the merge of the
rows of all views of an image on top of ``oracle.postprocess.mmcv_batched_nms`` (used as it is), and a second, brute-force
statement of the merge rule as plain loops.  Plain helper module, no pytest hooks; also the host merge of the "user's route"
leg of scripts/tta_bench.py."""
from __future__ import annotations

import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from oracle.postprocess import coordinate_offsets, mmcv_batched_nms  # noqa: E402

f32 = np.float32
FLIP_CODES = {None: 0, "horizontal": 1, "vertical": 2, "diagonal": 3}


def flip(img: np.ndarray, direction) -> np.ndarray:
    """mmcv ``imflip`` of [..., h, w, 3]: direction 1 / 'horizontal' = axis -2, 2 / 'vertical' = axis -3, 3 / 'diagonal' = both."""
    code = FLIP_CODES[direction] if isinstance(direction, (str, type(None))) else int(direction)
    out = img
    if code & 1:
        out = np.flip(out, axis=-2)
    if code & 2:
        out = np.flip(out, axis=-3)
    return np.ascontiguousarray(out)


def unflip_boxes(boxes: np.ndarray, code: int, w, h) -> np.ndarray:
    """mmdet ``bbox_flip`` with img_shape = ori_shape, one fp32 subtraction per coordinate."""
    b = np.array(boxes, f32, copy=True).reshape(-1, 4)
    W, H = f32(w), f32(h)
    if code & 1:
        b[:, 0], b[:, 2] = W - b[:, 2].copy(), W - b[:, 0].copy()
    if code & 2:
        b[:, 1], b[:, 3] = H - b[:, 3].copy(), H - b[:, 1].copy()
    return b


def survivors(boxes, scores, labels, counts, view_flip, wh, n_cls: int) -> dict:
    """Rows of ONE image ([V, max_in, ...], counts [V]) that pass the count / label filters, un-flipped, in slot order."""
    V, max_in = scores.shape
    b_, s_, l_, src_ = [], [], [], []
    for v in range(V):
        n = min(max(int(counts[v]), 0), max_in)
        ok = np.nonzero((labels[v, :n] >= 0) & (labels[v, :n] < n_cls))[0]
        b_.append(unflip_boxes(boxes[v, ok], int(view_flip[v]), wh[0], wh[1]))
        s_.append(scores[v, ok])
        l_.append(labels[v, ok].astype(np.int64))
        src_.append(v * max_in + ok)
    return dict(boxes=np.concatenate(b_).astype(f32).reshape(-1, 4), scores=np.concatenate(s_).astype(f32), labels=np.concatenate(l_),
                src=np.concatenate(src_).astype(np.int64))


def _iou(a: np.ndarray, b: np.ndarray) -> np.ndarray:
    """fp32 IoU of box ``a`` with boxes ``b``, every operation rounded (mmcv nms_cpu, offset 0)."""
    area_a = (a[2] - a[0]) * (a[3] - a[1])
    area_b = (b[:, 2] - b[:, 0]) * (b[:, 3] - b[:, 1])
    w = np.maximum(f32(0), np.minimum(a[2], b[:, 2]) - np.maximum(a[0], b[:, 0]))
    h = np.maximum(f32(0), np.minimum(a[3], b[:, 3]) - np.maximum(a[1], b[:, 1]))
    inter = w * h
    with np.errstate(divide="ignore", invalid="ignore"):
        return inter / (area_a + area_b - inter)


def merge(boxes, scores, labels, counts, view_flip, img_wh, n_cls: int, iou_thr: float, split_thr: int, max_out: int,
          witness: bool = True) -> dict:
    """``wd_views_merge``: boxes [V, B, max_in, 4], scores, labels [V, B, max_in], counts [V, B], view_flip [V], img_wh [B, 2] ->
    boxes [B, max_out, 4], scores, labels, src (int32, -1 filler), count [B], and two witnesses of what the case exercises:
    ``per_view`` [B, V] (output rows that came from each view) and ``cross_view`` [B] (rows suppressed by a kept row of ANOTHER
    view)."""
    boxes = np.asarray(boxes, f32)
    scores = np.asarray(scores, f32)
    labels = np.asarray(labels)
    counts = np.asarray(counts)
    V, B, max_in = scores.shape
    out = dict(boxes=np.zeros((B, max_out, 4), f32), scores=np.zeros((B, max_out), f32), labels=np.full((B, max_out), -1, np.int32),
               src=np.full((B, max_out), -1, np.int32), count=np.zeros(B, np.int32), per_view=np.zeros((B, V), np.int64),
               cross_view=np.zeros(B, np.int64))
    cfg = dict(type="nms", iou_threshold=iou_thr, split_thr=split_thr)
    for b in range(B):
        if bool((counts[:, b] < 0).any()):
            out["count"][b] = -1
            continue
        s = survivors(boxes[:, b], scores[:, b], labels[:, b], counts[:, b], view_flip, img_wh[b], n_cls)
        if not len(s["scores"]):
            continue
        order = np.argsort(-s["scores"], kind="stable")      # slot order is ascending already: (score desc, slot asc)
        bx, sc, lb, src = s["boxes"][order], s["scores"][order], s["labels"][order], s["src"][order]
        keep = mmcv_batched_nms(bx, sc, lb, cfg, max_keep=max_out)
        n = len(keep)
        W, H = f32(img_wh[b][0]), f32(img_wh[b][1])
        out["boxes"][b, :n] = np.clip(bx[keep], f32(0), np.asarray([W, H, W, H], f32))
        out["scores"][b, :n], out["labels"][b, :n], out["src"][b, :n], out["count"][b] = sc[keep], lb[keep], src[keep], n
        out["per_view"][b] = np.bincount(src[keep] // max_in, minlength=V)
        if not witness:
            continue
        # witness: rows the FULL NMS drops that a kept row of another view overlaps beyond the threshold
        full = mmcv_batched_nms(bx, sc, lb, cfg)
        kept = np.zeros(len(sc), bool)
        kept[full] = True
        off = coordinate_offsets(bx, lb)
        per_class = len(sc) >= split_thr
        vw = src // max_in
        for i in np.nonzero(~kept)[0]:
            prior = np.nonzero(kept[:i] & (vw[:i] != vw[i]) & ((lb[:i] == lb[i]) if per_class else True))[0]
            if prior.size and bool((_iou(off[i], off[prior]) > f32(iou_thr)).any()):
                out["cross_view"][b] += 1
    return out


def merge_brute(boxes, scores, labels, counts, view_flip, img_wh, n_cls: int, iou_thr: float, split_thr: int, max_out: int) -> list:
    """The rule of the header written as plain loops over fp32 scalars, without ``mmcv_batched_nms``: per image either -1 (a
    view tripped) or [(src, label, (x1, y1, x2, y2), score), ...]."""
    boxes, scores = np.asarray(boxes, f32), np.asarray(scores, f32)
    V, B, max_in = scores.shape
    thr = f32(iou_thr)
    res = []
    for b in range(B):
        if any(int(counts[v][b]) < 0 for v in range(V)):
            res.append(-1)
            continue
        W, H = f32(img_wh[b][0]), f32(img_wh[b][1])
        rows = []                                            # (score, slot, label, box)
        for v in range(V):
            for r in range(min(int(counts[v][b]), max_in)):
                lb = int(labels[v][b][r])
                if not 0 <= lb < n_cls:
                    continue
                x1, y1, x2, y2 = (f32(c) for c in boxes[v, b, r])
                if int(view_flip[v]) & 1:
                    x1, x2 = f32(W - x2), f32(W - x1)
                if int(view_flip[v]) & 2:
                    y1, y2 = f32(H - y2), f32(H - y1)
                rows.append((f32(scores[v, b, r]), v * max_in + r, lb, (x1, y1, x2, y2)))
        rows.sort(key=lambda t: (-float(t[0]), t[1]))
        if not rows:
            res.append([])
            continue
        step = f32(max(max(t[3]) for t in rows) + f32(1))
        per_class = len(rows) >= split_thr
        kept, kept_off = [], []
        for sc, slot, lb, bx in rows:
            o = f32(f32(lb) * step)
            c = tuple(f32(q + o) for q in bx)
            area = f32(f32(c[2] - c[0]) * f32(c[3] - c[1]))
            ok = True
            for (ksc, kslot, klb, kbx), (kc, karea) in zip(kept, kept_off):
                if per_class and klb != lb:
                    continue
                iw = max(f32(0), f32(min(kc[2], c[2]) - max(kc[0], c[0])))
                ih = max(f32(0), f32(min(kc[3], c[3]) - max(kc[1], c[1])))
                inter = f32(iw * ih)
                with np.errstate(divide="ignore", invalid="ignore"):
                    ovr = f32(inter / f32(f32(karea + area) - inter))
                if ovr > thr:
                    ok = False
                    break
            if ok:
                kept.append((sc, slot, lb, bx))
                kept_off.append((c, area))
                if len(kept) >= max_out:
                    break
        res.append([(slot, lb, tuple(float(min(max(q, f32(0)), lim)) for q, lim in zip(bx, (W, H, W, H))), float(sc))
                    for sc, slot, lb, bx in kept])
    return res


def brute_equals(out: dict, brute: list) -> bool:
    """``merge``'s outputs against ``merge_brute``'s lists, bit for bit."""
    for b, rows in enumerate(brute):
        n = int(out["count"][b])
        if rows == -1:
            if n != -1:
                return False
            continue
        if n != len(rows):
            return False
        got = [(int(out["src"][b, i]), int(out["labels"][b, i]), tuple(float(q) for q in out["boxes"][b, i]), float(out["scores"][b, i]))
               for i in range(n)]
        if got != rows:
            return False
    return True


# --------------------------------------------------------------------------------------------------------------------
# seeded merge inputs shared by tests/test_gpu_views.py, tests/test_gpu_views_extents.py and tests/test_cpu_views.py
# --------------------------------------------------------------------------------------------------------------------
NAN_BITS = 0x7FC01234          # what rows beyond a count hold (a NaN as fp32, a huge label as int32)


def image_sizes(B: int) -> np.ndarray:
    """[B, 2] fp32 (width, height), all odd: 641 x 427, 643 x 429, ..."""
    return np.asarray([[641 + 2 * (b % 7), 427 + 2 * (b % 5)] for b in range(B)], f32)


def merge_inputs(V: int, B: int, max_in: int, seed: int = 0, counts: str = "mixed", flips=None, n_cls: int = 80) -> dict:
    """boxes [V, B, max_in, 4], scores, labels, counts [V, B], view_flip [V], img_wh [B, 2] of a case.  Per image a set of
    objects (clustered: a few centres, boxes of 8 .. 60 pixels on a quarter-pixel grid) that every view sees with probability
    0.8, jittered by up to half a pixel and stored in the VIEW's coordinates (flipped by its code), so that the views' rows
    suppress each other; scores on a grid of 1/64 (equal scores across views: the slot decides); labels from
    {0, 1, 2, n_cls - 1}.  Planted in every view with rows: object 0 exactly (mirrored pairs, the score falls with the view
    index) and object 1 exactly with ONE score (a tie across views).  About one row in 16 carries a label outside [0, n_cls).
    Everything beyond a count holds NaN bits.  ``counts``: "mixed" ((v + b) % 3: full, partial, 0), "zero", "full"."""
    rng = np.random.default_rng(seed)
    flips = [(1, 0, 2, 3)[v % 4] for v in range(V)] if flips is None else list(flips)
    assert len(flips) == V
    wh = image_sizes(B)
    boxes = np.full((V, B, max_in, 4), NAN_BITS, np.uint32).view(f32)
    scores = np.full((V, B, max_in), NAN_BITS, np.uint32).view(f32)
    labels = np.full((V, B, max_in), NAN_BITS, np.int32)
    cnt = np.zeros((V, B), np.int32)
    label_set = sorted({0, min(1, n_cls - 1), min(2, n_cls - 1), n_cls - 1})
    for b in range(B):
        W, H = float(wh[b, 0]), float(wh[b, 1])
        n_obj = max(2, (2 * max_in) // 3)
        centres = rng.uniform(0.15, 0.85, (max(2, n_obj // 6), 2)) * (W, H)
        objs = []
        for k in range(n_obj):
            cx, cy = centres[k % len(centres)] + rng.normal(0, 25, 2)
            bw, bh = rng.integers(8, 61, 2)
            x1 = float(np.clip(np.round((cx - bw / 2) * 4) / 4, 0, W - bw))
            y1 = float(np.clip(np.round((cy - bh / 2) * 4) / 4, 0, H - bh))
            objs.append((x1, y1, x1 + float(bw), y1 + float(bh), int(rng.choice(label_set))))
        for v in range(V):
            if counts in ("zero", "full"):
                want = 0 if counts == "zero" else max_in
            else:
                want = (max_in, int(rng.integers(1, max_in + 1)), 0)[(v + b) % 3]
            if not want:
                continue
            rows = [(*objs[0][:4], 0.984375 - 0.015625 * v, objs[0][4]), (*objs[1][:4], 0.859375, objs[1][4])]
            for o in objs[2:]:
                if rng.random() < 0.8:
                    j = 0.25 * rng.integers(-2, 3, 4)
                    x1, y1 = max(o[0] + j[0], 0.0), max(o[1] + j[1], 0.0)
                    x2, y2 = min(max(o[2] + j[2], x1 + 1.0), W), min(max(o[3] + j[3], y1 + 1.0), H)
                    rows.append((x1, y1, x2, y2, float(rng.integers(1, 52)) / 64.0, o[4]))
            while len(rows) < want:
                bw, bh = rng.integers(8, 61, 2)
                x1, y1 = 0.25 * rng.integers(0, int(4 * (W - bw)) + 1), 0.25 * rng.integers(0, int(4 * (H - bh)) + 1)
                rows.append((x1, y1, x1 + float(bw), y1 + float(bh), float(rng.integers(1, 52)) / 64.0, int(rng.choice(label_set))))
            rows = sorted(rows, key=lambda r: -r[4])[:want]          # a step's rows: score descending
            cnt[v, b] = len(rows)
            for r, row in enumerate(rows):
                x1, y1, x2, y2 = row[:4]
                if flips[v] & 1:
                    x1, x2 = W - x2, W - x1                  # exact: quarter pixels, W an integer
                if flips[v] & 2:
                    y1, y2 = H - y2, H - y1
                boxes[v, b, r] = (x1, y1, x2, y2)
                scores[v, b, r] = row[4]
                labels[v, b, r] = row[5]
                if r >= 2 and rng.random() < 1 / 16:
                    labels[v, b, r] = (n_cls, -1, 2 ** 30)[int(rng.integers(0, 3))]
    return dict(boxes=boxes, scores=scores, labels=labels, counts=cnt, view_flip=np.asarray(flips, np.int32), img_wh=wh)


# --------------------------------------------------------------------------------------------------------------------
# the whole path on the plain API (tests/test_gpu_views.py, scripts/tta_bench.py); needs a device
# --------------------------------------------------------------------------------------------------------------------
def _view_code(samples) -> int:
    codes = set()
    for s in samples:
        m = s.metainfo if hasattr(s, "metainfo") else s
        codes.add(FLIP_CODES[m.get("flip_direction")] if m.get("flip") else 0)
    assert len(codes) == 1
    return codes.pop()


def user_route(model, views, tta_cfg, witness=True) -> dict:
    """What a caller of the plain API does: ``predict`` per view, every view's rows downloaded, the un-flip and the merge in
    numpy (``merge``).  ``views``: [(batch_inputs, batch_data_samples), ...]."""
    V, B = len(views), len(views[0][1])
    max_in = model._h.max_out
    boxes = np.zeros((V, B, max_in, 4), np.float32)
    scores = np.zeros((V, B, max_in), np.float32)
    labels = np.full((V, B, max_in), -1, np.int32)
    counts = np.zeros((V, B), np.int32)
    flips = np.zeros(V, np.int32)
    wh = np.zeros((B, 2), np.float32)
    n_cls = 0
    for v, (inputs, samples) in enumerate(views):
        flips[v] = _view_code(samples)
        for b, s in enumerate(model.predict(inputs, [type(s)(metainfo=s.metainfo) for s in samples])):
            p = s.pred_instances
            n = len(p.scores)
            boxes[v, b, :n], scores[v, b, :n] = p.bboxes.cpu().numpy(), p.scores.cpu().numpy()
            labels[v, b, :n], counts[v, b] = p.labels.cpu().numpy(), n
            if v == 0:
                ori = s.metainfo["ori_shape"]
                wh[b] = (ori[1], ori[0])
                n_cls = max(n_cls, int(model._bank_for(s).shape[0]))
    nms = tta_cfg["nms"]
    out = merge(boxes, scores, labels, counts, flips, wh, n_cls, nms["iou_threshold"], int(nms.get("split_thr", 10000)),
                int(tta_cfg["max_per_img"]), witness=witness)
    out["per_view_in"] = counts
    return out
