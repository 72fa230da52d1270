"""Tile plans of the tiled inference path (host, numpy only): which overlapping network-sized windows of a large image are
detected on, and how each of them sits in the image.  The plan is a structured array whose dtype is ``struct WdTile``
(include/wedetect_hip_tile.h; ``wedetect_amd/tile.py`` asserts the size against the library): it is uploaded as it is and
read by ``wd_tile_cut_u8`` and ``wd_tile_merge``.

Grid along one axis (x; y alike), for a tile width ``tw`` and ``overlap`` in [0, 0.5]:

    ov = int(tw * overlap); stride = tw - ov
    W <= tw :  one column at x0 = 0 with valid width W
    else    :  nx = ceil((W - tw) / stride) + 1,  x0_i = min(i * stride, W - tw)      (the last tile is shifted inward:
               every tile is full)

Tiles are row-major; with ``overview`` and more than one crop ONE overview tile is appended last: the whole image through
the shipped test pipeline's geometry (``overview_geometry``), which catches the objects larger than the overlap.
"""
from __future__ import annotations

from typing import Tuple

import numpy as np

CROP, OVERVIEW, BLANK = 0, 1, 2
LEFT, TOP, RIGHT, BOTTOM = 1, 2, 4, 8

TILE_FIELDS = ("x0", "y0", "w", "h", "interior_mask", "kind", "img_w", "img_h")
TILE_DTYPE = np.dtype([(n, "<i4") for n in TILE_FIELDS], align=True)


def _axis(size: int, tile: int, overlap: float):
    """[(origin, valid length), ...] of the tiles along one axis."""
    if size <= tile:
        return [(0, size)]
    ov = int(tile * overlap)
    stride = tile - ov
    n = -(-(size - tile) // stride) + 1
    return [(min(i * stride, size - tile), tile) for i in range(n)]


def _check(h: int, w: int, tile, overlap: float) -> Tuple[int, int]:
    if not (isinstance(tile, (tuple, list)) and len(tile) == 2):
        raise TypeError("tile must be an (h, w) pair")
    th, tw = int(tile[0]), int(tile[1])
    if th < 32 or tw < 32 or th % 32 or tw % 32:
        raise ValueError(f"tile size {th}x{tw} is not a positive multiple of 32")
    if not 0.0 <= float(overlap) <= 0.5:
        raise ValueError("overlap must lie in [0, 0.5]")
    if int(h) < 1 or int(w) < 1:
        raise ValueError("empty image")
    return th, tw


def plan_tiles(h: int, w: int, tile=(640, 640), overlap: float = 0.2, overview: bool = True) -> np.ndarray:
    """The plan of an ``h x w`` image: a ``TILE_DTYPE`` array, deterministic.  An image that fits one tile gives ONE crop with
    no interior side (``fits_one_tile``): the caller runs the plain step on it."""
    th, tw = _check(h, w, tile, overlap)
    h, w = int(h), int(w)
    xs, ys = _axis(w, tw, float(overlap)), _axis(h, th, float(overlap))
    n = len(xs) * len(ys)
    plan = np.zeros(n + (1 if overview and n > 1 else 0), TILE_DTYPE)
    plan["img_w"], plan["img_h"] = w, h
    k = 0
    for y0, vh in ys:
        for x0, vw in xs:
            t = plan[k]
            t["x0"], t["y0"], t["w"], t["h"], t["kind"] = x0, y0, vw, vh, CROP
            t["interior_mask"] = (LEFT * (x0 > 0) | TOP * (y0 > 0) | RIGHT * (x0 + vw < w) | BOTTOM * (y0 + vh < h))
            k += 1
    if k < len(plan):
        t = plan[k]
        t["w"], t["h"], t["kind"] = w, h, OVERVIEW          # no interior side, no offset: its rows are in image pixels
    return plan


def fits_one_tile(plan: np.ndarray) -> bool:
    return len(plan) == 1 and int(plan[0]["kind"]) == CROP and int(plan[0]["interior_mask"]) == 0


def n_crops(plan: np.ndarray) -> int:
    return int((plan["kind"] == CROP).sum())


def pad_plan(plan: np.ndarray, n: int) -> np.ndarray:
    """``plan`` followed by blank tiles up to ``n`` (batch padding)."""
    if n < len(plan):
        raise ValueError("a plan cannot shrink")
    out = np.zeros(n, TILE_DTYPE)
    out[: len(plan)] = plan
    out["kind"][len(plan):] = BLANK
    out["img_w"], out["img_h"] = plan["img_w"][0], plan["img_h"][0]
    return out


def step_sizes(n_tile: int, tile_batch: int):
    """Tower batch sizes of the steps ``n_tile`` tiles run in: full steps of ``tile_batch``, then the remainder ``r`` on the
    tower of the next power of two >= r, padded with blank tiles.  [(tiles, tower batch), ...]"""
    if tile_batch < 1:
        raise ValueError("tile_batch must be positive")
    out = [(tile_batch, tile_batch)] * (n_tile // tile_batch)
    r = n_tile % tile_batch
    if r:
        b = 1
        while b < r:
            b <<= 1
        out.append((r, b))
    return out


def overview_geometry(h: int, w: int, tile=(640, 640)) -> dict:
    """The overview tile: the whole image through ``WeDetectKeepRatioResize`` + ``WeDetectLetterResize`` (allow_scale_up=False,
    pad 114) to ``tile`` — the transforms' own geometry code runs (wedetect_amd/pipeline.py), nothing is restated.  Returns
    what the resample needs (``dh, dw, interp, top, left, pad_val``) and the post-process's ``meta`` (8 floats)."""
    from .detector import letterbox_meta
    from .pipeline import WeDetectKeepRatioResize, WeDetectLetterResize
    th, tw = int(tile[0]), int(tile[1])
    r = dict(img_shape=(int(h), int(w)), ori_shape=(int(h), int(w)))
    r = WeDetectKeepRatioResize(scale=(tw, th))(r)
    g = WeDetectLetterResize(scale=(tw, th), allow_scale_up=False, pad_val=dict(img=114)).geometry(r, (int(h), int(w)))
    g["meta"] = letterbox_meta(dict(ori_shape=(int(h), int(w)), scale_factor=r["scale_factor"], pad_param=r["pad_param"]), th, tw, True)
    g["pad_param"], g["scale_factor"] = r["pad_param"], r["scale_factor"]
    return g


def tile_meta(plan: np.ndarray, tile, overview_meta=None) -> np.ndarray:
    """[n, 8] float32 post-process metadata of the tiles: ``{0, 0, 0, 1, 1, w, h, 1}`` for crops (and blanks, whose rows are
    never read), the pipeline's own for the overview."""
    out = np.zeros((len(plan), 8), np.float32)
    out[:, 3] = out[:, 4] = out[:, 7] = 1.0
    out[:, 5], out[:, 6] = plan["w"], plan["h"]
    blank = plan["kind"] == BLANK
    out[blank, 5], out[blank, 6] = float(tile[1]), float(tile[0])
    for i in np.nonzero(plan["kind"] == OVERVIEW)[0]:
        if overview_meta is None:
            raise ValueError("the plan has an overview tile: its metadata is needed")
        out[i] = np.asarray(overview_meta, np.float32)
    return out
