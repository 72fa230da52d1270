"""Numpy restatement of the tiled inference path (include/wedetect_hip_tile.h): the cut by slicing, the merge on top of
``oracle.postprocess.mmcv_batched_nms`` (used as it is).  Plain helper module, no pytest hooks; also the host merge of the
"user's route" leg of scripts/tiled_bench.py."""
from __future__ import annotations

import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from oracle.postprocess import coordinate_offsets, mmcv_batched_nms  # noqa: E402

f32 = np.float32
CROP, OVERVIEW, BLANK = 0, 1, 2


def cut(img: np.ndarray, plan: np.ndarray, tile, fill: int = 114, swap_rb: bool = False, dst: np.ndarray = None) -> np.ndarray:
    """[n, th, tw, 3] tiles of ``img`` (uint8 HWC); overview slots keep what ``dst`` held (zeros without one)."""
    th, tw = tile
    out = np.zeros((len(plan), th, tw, 3), np.uint8) if dst is None else dst.copy()
    for k, t in enumerate(plan):
        if t["kind"] == OVERVIEW:
            continue
        out[k] = fill
        if t["kind"] == CROP:
            win = img[t["y0"]:t["y0"] + t["h"], t["x0"]:t["x0"] + t["w"]]
            out[k, :t["h"], :t["w"]] = win[:, :, ::-1] if swap_rb else win
    return out


def survivors(boxes, scores, labels, counts, plan, n_cls: int, edge_margin: float) -> dict:
    """Rows that pass the count / label / border filters, translated to image pixels, in slot order.  ``dropped`` counts the
    border drops."""
    n_tile, max_in = scores.shape
    m = f32(edge_margin)
    b_, s_, l_, src_, tile_ = [], [], [], [], []
    dropped = 0
    for t in range(n_tile):
        d = plan[t]
        if d["kind"] == BLANK:
            continue
        for r in range(min(max(int(counts[t]), 0), max_in)):
            lb = int(labels[t, r])
            if not 0 <= lb < n_cls:
                continue
            x1, y1, x2, y2 = (f32(v) for v in boxes[t, r])
            if d["kind"] == CROP:
                w, h, k = f32(d["w"]), f32(d["h"]), int(d["interior_mask"])
                if m > 0 and ((k & 1 and x1 < m) or (k & 2 and y1 < m) or (k & 4 and x2 > f32(w - m)) or (k & 8 and y2 > f32(h - m))):
                    dropped += 1
                    continue
                fx, fy = f32(d["x0"]), f32(d["y0"])
                x1, y1, x2, y2 = f32(x1 + fx), f32(y1 + fy), f32(x2 + fx), f32(y2 + fy)
            b_.append((x1, y1, x2, y2))
            s_.append(scores[t, r])
            l_.append(lb)
            src_.append(t * max_in + r)
            tile_.append(t)
    return dict(boxes=np.asarray(b_, f32).reshape(-1, 4), scores=np.asarray(s_, f32), labels=np.asarray(l_, np.int64),
                src=np.asarray(src_, np.int64), tile=np.asarray(tile_, np.int64), dropped=dropped)


def _iou(a: np.ndarray, b: np.ndarray) -> np.ndarray:
    """fp32 IoU of box ``a`` with boxes ``b``, every operation rounded (mmcv nms_cpu, offset 0)."""
    area_a = (a[2] - a[0]) * (a[3] - a[1])
    area_b = (b[:, 2] - b[:, 0]) * (b[:, 3] - b[:, 1])
    w = np.maximum(f32(0), np.minimum(a[2], b[:, 2]) - np.maximum(a[0], b[:, 0]))
    h = np.maximum(f32(0), np.minimum(a[3], b[:, 3]) - np.maximum(a[1], b[:, 1]))
    inter = w * h
    with np.errstate(divide="ignore", invalid="ignore"):
        return inter / (area_a + area_b - inter)


def merge(boxes, scores, labels, counts, plan, n_cls: int, edge_margin: float, iou_thr: float, split_thr: int, max_out: int,
          witness: bool = True) -> dict:
    """``wd_tile_merge``: -> boxes [max_out, 4], scores, labels, src (int32, -1 filler), count, and two witnesses of what the
    case exercises: ``dropped`` (border drops) and ``cross_tile`` (rows suppressed by a kept row of ANOTHER tile)."""
    boxes = np.asarray(boxes, f32)
    scores = np.asarray(scores, f32)
    labels = np.asarray(labels)
    counts = np.asarray(counts)
    out = dict(boxes=np.zeros((max_out, 4), f32), scores=np.zeros(max_out, f32), labels=np.full(max_out, -1, np.int32),
               src=np.full(max_out, -1, np.int32), count=0, dropped=0, cross_tile=0)
    if any(int(counts[t]) < 0 for t in range(len(plan)) if plan[t]["kind"] != BLANK):
        out["count"] = -1
        return out
    s = survivors(boxes, scores, labels, counts, plan, n_cls, edge_margin)
    out["dropped"] = s["dropped"]
    if not len(s["scores"]):
        return out
    order = np.argsort(-s["scores"], kind="stable")          # slot order is ascending already: (score desc, slot asc)
    b, sc, lb, src, tl = s["boxes"][order], s["scores"][order], s["labels"][order], s["src"][order], s["tile"][order]
    cfg = dict(type="nms", iou_threshold=iou_thr, split_thr=split_thr)
    keep = mmcv_batched_nms(b, sc, lb, cfg, max_keep=max_out)
    n = len(keep)
    W, H = f32(plan[0]["img_w"]), f32(plan[0]["img_h"])
    out["boxes"][:n] = np.clip(b[keep], f32(0), np.asarray([W, H, W, H], f32))
    out["scores"][:n], out["labels"][:n], out["src"][:n], out["count"] = sc[keep], lb[keep], src[keep], n
    if not witness:
        return out
    # witness: rows the FULL NMS drops that a kept row of another tile overlaps beyond the threshold
    full = mmcv_batched_nms(b, sc, lb, cfg)
    kept = np.zeros(len(sc), bool)
    kept[full] = True
    off = coordinate_offsets(b, lb)
    per_class = len(sc) >= split_thr
    for i in np.nonzero(~kept)[0]:
        prior = np.nonzero(kept[:i] & (tl[:i] != tl[i]) & ((lb[:i] == lb[i]) if per_class else True))[0]
        if prior.size and bool((_iou(off[i], off[prior]) > f32(iou_thr)).any()):
            out["cross_tile"] += 1
    return out


def merge_brute(boxes, scores, labels, counts, plan, n_cls: int, edge_margin: float, iou_thr: float, max_out: int) -> list:
    """The agnostic branch as a plain double loop over python floats promoted from fp32 (tests/test_cpu_tile.py checks
    ``merge`` against it on hand-made vectors whose IoUs are far from the threshold).  -> [(src, label), ...]"""
    s = survivors(np.asarray(boxes, f32), np.asarray(scores, f32), np.asarray(labels), np.asarray(counts), plan, n_cls, edge_margin)
    rows = sorted(range(len(s["scores"])), key=lambda i: (-float(s["scores"][i]), int(s["src"][i])))
    if not rows:
        return []
    step = float(s["boxes"].max()) + 1.0
    kept = []
    for i in rows:
        bi = [float(v) + float(s["labels"][i]) * step for v in s["boxes"][i]]
        ok = True
        for j in kept:
            bj = [float(v) + float(s["labels"][j]) * step for v in s["boxes"][j]]
            iw = max(0.0, min(bi[2], bj[2]) - max(bi[0], bj[0]))
            ih = max(0.0, min(bi[3], bj[3]) - max(bi[1], bj[1]))
            inter = iw * ih
            union = (bi[2] - bi[0]) * (bi[3] - bi[1]) + (bj[2] - bj[0]) * (bj[3] - bj[1]) - inter
            if union > 0 and inter / union > iou_thr:
                ok = False
                break
        if ok:
            kept.append(i)
            if len(kept) >= max_out:
                break
    return [(int(s["src"][i]), int(s["labels"][i])) for i in kept]


# --------------------------------------------------------------------------------------------------------------------
# hand-made merge inputs shared by tests/test_gpu_tile.py, tests/test_gpu_tile_extents.py and tests/test_cpu_tile.py
# --------------------------------------------------------------------------------------------------------------------
N_CLS = 1203
NAN_BITS = 0x7FC01234          # what rows beyond a tile's count hold (a NaN as fp32, a huge label as int32)


def case_plan(n_tile: int) -> tuple:
    """(plan of ``n_tile`` descriptors, tile) for the shapes the tests use: 64 x 64 tiles; 1 = an image that is one tile,
    3 = 2 crops + overview, 9 = 8 crops + overview, 128 = 10 x 12 crops + overview + 7 blank tiles."""
    from wedetect_amd import tiling as G
    tile = (64, 64)
    if n_tile == 1:
        return G.plan_tiles(50, 64, tile, 0.25), tile
    if n_tile == 3:
        return G.plan_tiles(64, 112, tile, 0.25), tile
    if n_tile == 9:
        return G.plan_tiles(96, 160, tile, 0.5), tile
    if n_tile == 128:
        return G.pad_plan(G.plan_tiles(496, 592, tile, 0.25), 128), tile
    raise ValueError(n_tile)


def merge_inputs(n_tile: int, max_in: int, seed: int = 0, counts: str = "mixed") -> dict:
    """boxes [n_tile, max_in, 4], scores, labels, counts of a case.  Per tile: random boxes inside the valid window (some
    touching its sides: border drops), scores on a coarse grid (equal scores across tiles: the slot decides), labels from
    {0, 1, 2, 1202}; in every pair of horizontally overlapping crops one object seen by both (IoU 1: the lower score goes)
    and one pair of boxes of IoU ~0.6 (both stay at 0.7), once with label 1202 (offsets of ~7e5: fp32 steps of 1/16 pixel);
    the overview repeats an object of crop 0.  Everything beyond a tile's count, and all of a blank tile, holds NaN bits.
    ``counts``: "mixed" (0, full and in between), "zero", "full"."""
    plan, tile = case_plan(n_tile)
    assert len(plan) == n_tile
    rng = np.random.default_rng(seed)
    boxes = np.full((n_tile, max_in, 4), NAN_BITS, np.uint32).view(f32)
    scores = np.full((n_tile, max_in), NAN_BITS, np.uint32).view(f32)
    labels = np.full((n_tile, max_in), NAN_BITS, np.int32)
    cnt = np.zeros(n_tile, np.int32)
    rows = [[] for _ in range(n_tile)]                       # (x1, y1, x2, y2, score, label), tile-local
    crops = [t for t in range(n_tile) if plan[t]["kind"] == CROP]
    for a in crops:                                          # planted pairs across the overlap with the right neighbour
        b = a + 1
        if b not in crops or plan[b]["y0"] != plan[a]["y0"] or plan[b]["x0"] >= plan[a]["x0"] + plan[a]["w"] - 14:
            continue
        ox0, oy0 = int(plan[b]["x0"]) + 3, int(plan[a]["y0"]) + 5          # image pixels, > margin away from both sides
        lab = 1202 if a % 2 else 1
        for k, (dx, dy, sa, sb) in enumerate(((0.0, 0.0, 0.9140625, 0.8828125), (2.5, 0.0, 0.8515625, 0.8203125))):
            for t, sc, sx in ((a, sa, 0.0), (b, sb, dx)):    # second pair: shifted by 2.5 of 10 -> IoU 0.6
                lx, ly = ox0 + sx - plan[t]["x0"], oy0 + 14 * k + dy - plan[t]["y0"]
                rows[t].append((lx, ly, lx + 10.0, ly + 8.0 + 0.25 * k, sc, lab))
    for t in range(n_tile):                                  # an object of crop 0 that the overview sees too (image pixels)
        if plan[t]["kind"] == OVERVIEW and crops:
            rows[t].append((3.0, 4.0, 15.0, 13.0, 0.9765625, 2))
            rows[crops[0]].append((3.0, 4.0, 15.0, 13.0, 0.9453125, 2))
    for t in range(n_tile):
        d = plan[t]
        if d["kind"] == BLANK:
            cnt[t] = max_in                                  # a blank tile's count is never read either
            continue
        w, h = int(d["w"]), int(d["h"])                      # the valid window; the whole image for the overview
        if counts in ("zero", "full"):
            want = 0 if counts == "zero" else max_in
        elif n_tile < 128:
            want = (0 if n_tile >= 9 else 2, max_in, int(rng.integers(1, max_in + 1)))[(t + 2) % 3]
        else:                                                # the cap: two full tiles, the others short
            want = max_in if t in (5, 77) else int(rng.integers(0, min(max_in, 24) + 1))
        while len(rows[t]) < want:
            bw, bh = rng.integers(6, 24, 2)
            x1, y1 = rng.integers(0, max(w - bw, 1)), rng.integers(0, max(h - bh, 1))
            if rng.random() < 0.15:                          # touching the right / bottom side of the window
                x1, y1 = w - bw, (y1 if rng.random() < 0.5 else h - bh)
            q = 0.25 * rng.integers(0, 4, 4)
            sc = float(rng.integers(1, 64)) / 64.0
            rows[t].append((x1 + q[0], y1 + q[1], min(x1 + bw + q[2], w), min(y1 + bh + q[3], h), sc, int(rng.choice([0, 1, 2, 1202]))))
        rs = sorted(rows[t][:max_in], key=lambda r: -r[4]) if want else []      # a step's rows: score descending
        cnt[t] = len(rs)
        for r, row in enumerate(rs):
            boxes[t, r] = row[:4]
            scores[t, r] = row[4]
            labels[t, r] = row[5]
    return dict(plan=plan, tile=tile, boxes=boxes, scores=scores, labels=labels, counts=cnt)


# --------------------------------------------------------------------------------------------------------------------
# the whole path on the plain API (tests/test_gpu_tile.py, scripts/tiled_bench.py); needs a device
# --------------------------------------------------------------------------------------------------------------------
def pipeline_canvas(img_rgb, tile):
    """The image through the shipped test pipeline's own transforms -> (device HWC BGR canvas, metainfo)."""
    from wedetect_amd.pipeline import LoadImageFromFile, WeDetectKeepRatioResize, WeDetectLetterResize
    th, tw = tile
    r = LoadImageFromFile()(dict(img=np.ascontiguousarray(img_rgb[:, :, ::-1])))
    r = WeDetectKeepRatioResize(scale=(tw, th))(r)
    r = WeDetectLetterResize(scale=(tw, th), allow_scale_up=False, pad_val=dict(img=114))(r)
    return r["img"], dict(ori_shape=tuple(img_rgb.shape[:2]), scale_factor=r["scale_factor"], pad_param=r["pad_param"])


def user_route(model, img_rgb, tile, overlap, overview, tile_batch, edge_margin, n_cls, witness=True):
    """What a caller of the plain API does: host crops (the overview through the test pipeline), ``predict`` on the same groups
    (so that the same towers run), every tile's rows downloaded, the merge in numpy (tile_ref)."""
    import torch
    from wedetect_amd import tiling as G
    from wedetect_amd.detector import DetDataSample
    H, W = img_rgb.shape[:2]
    th, tw = tile
    plan = G.plan_tiles(H, W, tile, overlap, overview)
    steps = G.step_sizes(len(plan), tile_batch)
    total = sum(b for _, b in steps)
    plan = G.pad_plan(plan, total)
    tiles = cut(img_rgb, plan, tile)
    max_in = model._h.max_out
    boxes = np.zeros((total, max_in, 4), np.float32)
    scores = np.zeros((total, max_in), np.float32)
    labels = np.full((total, max_in), -1, np.int32)
    counts = np.zeros(total, np.int32)
    lo = 0
    for _, b in steps:
        inputs, samples = [], []
        for k in range(lo, lo + b):
            d = plan[k]
            if d["kind"] == G.OVERVIEW:
                canvas, meta = pipeline_canvas(img_rgb, tile)
                inputs.append(canvas.permute(2, 0, 1).contiguous())
            else:
                inputs.append(torch.from_numpy(np.ascontiguousarray(tiles[k][:, :, ::-1])).permute(2, 0, 1).contiguous())
                vh, vw = (th, tw) if d["kind"] == G.BLANK else (int(d["h"]), int(d["w"]))
                meta = dict(ori_shape=(vh, vw), scale_factor=(1.0, 1.0), pad_param=np.zeros(4, np.float32))
            samples.append(DetDataSample(metainfo=meta))
        for k, s in enumerate(model.predict(inputs, samples)):
            p = s.pred_instances
            n = len(p.scores)
            boxes[lo + k, :n], scores[lo + k, :n] = p.bboxes.cpu().numpy(), p.scores.cpu().numpy()
            labels[lo + k, :n], counts[lo + k] = p.labels.cpu().numpy(), n
        lo += b
    cfg = model.test_cfg
    out = merge(boxes, scores, labels, counts, plan, n_cls, edge_margin, cfg["nms"]["iou_threshold"],
                int(cfg["nms"].get("split_thr", 10000)), int(cfg["max_per_img"]), witness=witness)
    out["per_tile"] = counts
    return out
