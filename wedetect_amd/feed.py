"""ctypes binding of the batched ragged pre-processing entry points (include/wedetect_hip_feed.h, csrc/feed.hip) and the
host packing that goes with them.

One batch = one pinned "control block" — ``batch`` descriptors (``struct WdFeedImage``) followed, at a 256-byte
boundary, by the table arena — uploaded in ONE copy, plus the pixel arena.  The tables stay host arithmetic: the cached
``pipeline._area_table`` / ``_linear_table`` (through ``pipeline.resize_plan``) and ``preprocess.resample_coeffs``; within a
batch every distinct table is packed once (images of one size share them).

The packing (``plan_cv`` / ``plan_pillow`` -> ``pack_batch``) is numpy only, so it is testable without a device
(tests/test_cpu_feed.py interprets the packed format and compares with the oracle).
"""
from __future__ import annotations

import ctypes as C
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np

from . import lib as L
from .lib import i32, i64, vp

FEED_ABI_VERSION = 1
FEED_PILLOW = 4
ALIGN = 256                      # images in the pixel arena, the table arena in the control block, tmp ranges

SIGNATURES = {
    "wd_feed_abi_version": (None, []),
    "wd_feed_sizeof_image": (i32, []),
    "wd_feed_tmp_bytes": (i64, [i32, i32]),
    "wd_feed_batch_u8": (None, [vp, i64, vp, vp, i32, vp, i64, vp, i64, vp, i32, i32, vp]),
}
EXPORTS = tuple(SIGNATURES)


class FeedImage(C.Structure):
    """Mirror of ``struct WdFeedImage``."""
    _fields_ = [
        ("src_off", C.c_int64), ("tmp_off", C.c_int64),
        ("sh", C.c_int32), ("sw", C.c_int32), ("new_h", C.c_int32), ("new_w", C.c_int32), ("top", C.c_int32), ("left", C.c_int32),
        ("fill", C.c_int32), ("swap_rb", C.c_int32), ("mode", C.c_int32),
        ("xa", C.c_int32), ("xidx", C.c_int32), ("xw", C.c_int32), ("ya", C.c_int32), ("yidx", C.c_int32), ("yw", C.c_int32),
        ("ksize_h", C.c_int32), ("ksize_v", C.c_int32),
        ("p0", C.c_int32), ("p1", C.c_int32), ("p2", C.c_float),
    ]


IMAGE_DTYPE = np.dtype([(n, {C.c_int64: "<i8", C.c_int32: "<i4", C.c_float: "<f4"}[t]) for n, t in FeedImage._fields_], align=True)
TABLE_FIELDS = ("xa", "xidx", "xw", "ya", "yidx", "yw")


LIB = L.bind("feed", FEED_ABI_VERSION, SIGNATURES)
if not (LIB.wd_feed_sizeof_image() == C.sizeof(FeedImage) == IMAGE_DTYPE.itemsize):
    raise L.WedetectHipMissing("struct WdFeedImage layout differs between the library and feed.FeedImage; rebuild")


def _up(n: int, a: int = ALIGN) -> int:
    return (int(n) + a - 1) // a * a


def tmp_bytes(sh: int, new_w: int) -> int:
    return int(LIB.wd_feed_tmp_bytes(int(sh), int(new_w)))


def fill_rgb(c0: int, c1: Optional[int] = None, c2: Optional[int] = None) -> int:
    """The descriptor's ``fill``: one byte per canvas channel."""
    c1 = c0 if c1 is None else c1
    c2 = c0 if c2 is None else c2
    for v in (c0, c1, c2):
        if not 0 <= int(v) <= 255:
            raise ValueError("fill values are bytes")
    return int(c0) | int(c1) << 8 | int(c2) << 16


# --------------------------------------------------------------------------------------------------
# plans: what one image needs, host side (geometry + the keys and arrays of its tables)
# --------------------------------------------------------------------------------------------------
def plan_cv(sh: int, sw: int, new_h: int, new_w: int, interp: str, top: int, left: int, fill: int = 114,
            swap_rb: bool = False) -> dict:
    """An image of the OpenCV family (the mmdet test pipeline): ``pipeline.resize_plan`` decides the mode."""
    from .pipeline import resize_plan
    p = resize_plan(sh, sw, new_h, new_w, interp)
    tables = {}
    if p["mode"] == L.CVRESIZE_AREA:
        tables = dict(xa=(("area", sw, new_w, "r"), p["xa"]), xidx=(("area", sw, new_w, "i"), p["xidx"]),
                      xw=(("area", sw, new_w, "w"), p["xw"]), ya=(("area", sh, new_h, "r"), p["ya"]),
                      yidx=(("area", sh, new_h, "i"), p["yidx"]), yw=(("area", sh, new_h, "w"), p["yw"]))
    elif p["mode"] == L.CVRESIZE_LINEAR:
        tables = dict(xa=(("lin", sw, new_w, True, "c"), p["xa"]), xidx=(("lin", sw, new_w, True, "i"), p["xidx"]),
                      ya=(("lin", sh, new_h, False, "c"), p["ya"]), yidx=(("lin", sh, new_h, False, "i"), p["yidx"]))
    return dict(mode=int(p["mode"]), sh=int(sh), sw=int(sw), new_h=int(new_h), new_w=int(new_w), top=int(top), left=int(left),
                fill=fill_rgb(fill), swap_rb=int(bool(swap_rb)), p0=int(p.get("p0", 0)), p1=int(p.get("p1", 0)),
                p2=float(p.get("p2", 0.0)), ksize_h=0, ksize_v=0, tables=tables, tmp_bytes=0)


def plan_pillow(sh: int, sw: int, new_h: int, new_w: int, top: int, left: int, fill=(114, 114, 114), swap_rb: bool = False) -> dict:
    """An image of the Pillow family (two-pass antialiased BILINEAR, ``preprocess.resample_coeffs``)."""
    from .preprocess import resample_coeffs
    bh, kh = resample_coeffs(sw, new_w)
    bv, kv = resample_coeffs(sh, new_h)
    tables = dict(xa=(("pil", sw, new_w, "b"), bh), xidx=(("pil", sw, new_w, "k"), kh),
                  ya=(("pil", sh, new_h, "b"), bv), yidx=(("pil", sh, new_h, "k"), kv))
    return dict(mode=FEED_PILLOW, sh=int(sh), sw=int(sw), new_h=int(new_h), new_w=int(new_w), top=int(top), left=int(left),
                fill=fill_rgb(*fill), swap_rb=int(bool(swap_rb)), p0=0, p1=0, p2=0.0, ksize_h=int(kh.shape[1]),
                ksize_v=int(kv.shape[1]), tables=tables, tmp_bytes=tmp_bytes(sh, new_w))


def src_offsets(shapes: Sequence[Tuple[int, int]]) -> Tuple[List[int], int]:
    """256-byte aligned offsets of images [(h, w), ...] in the pixel arena, and the arena bytes they take."""
    offs, top = [], 0
    for h, w in shapes:
        offs.append(top)
        top = _up(top + int(h) * int(w) * 3)
    return offs, max(top, ALIGN)


def control_bytes(plans: Sequence[dict]) -> Tuple[int, int, int]:
    """(bytes of the control block, byte offset of its table arena, table elements) of a batch."""
    seen, elems = set(), 0
    for p in plans:
        for key, arr in p["tables"].values():
            if key not in seen:
                seen.add(key)
                elems += int(arr.size)
    tab_off = _up(len(plans) * IMAGE_DTYPE.itemsize)
    return tab_off + _up(4 * elems), tab_off, elems


def pack_batch(plans: Sequence[dict], offsets: Sequence[int], out: Optional[np.ndarray] = None) -> dict:
    """Writes the control block of a batch into ``out`` (uint8, e.g. a view of pinned memory; allocated when None):
    descriptors at 0, the deduplicated tables from ``tab_off`` on.  Returns ``block`` (the bytes written), ``images`` (a
    structured view of the descriptors), ``tables`` (an int32 view of the table arena; float tables keep their bits),
    ``tab_off``, ``table_elems``, ``tmp_bytes`` (the tmp arena this batch needs) and ``n_tables`` (distinct tables packed)."""
    total, tab_off, elems = control_bytes(plans)
    if out is None:
        out = np.zeros(total, np.uint8)
    if out.dtype != np.uint8 or out.ndim != 1 or out.size < total:
        raise ValueError(f"control block needs {total} bytes")
    block = out[:total]
    images = block[: len(plans) * IMAGE_DTYPE.itemsize].view(IMAGE_DTYPE)
    tables = block[tab_off: tab_off + 4 * elems].view(np.int32)
    where: Dict[tuple, int] = {}
    top = tmp_top = 0
    for i, (p, off) in enumerate(zip(plans, offsets)):
        d = images[i]
        for f in ("sh", "sw", "new_h", "new_w", "top", "left", "fill", "swap_rb", "mode", "ksize_h", "ksize_v", "p0", "p1", "p2"):
            d[f] = p[f]
        d["src_off"] = int(off)
        for f in TABLE_FIELDS:
            d[f] = -1
        for f, (key, arr) in p["tables"].items():
            at = where.get(key)
            if at is None:
                at = where[key] = top
                flat = np.ascontiguousarray(arr).reshape(-1)
                if flat.dtype.itemsize != 4:
                    raise TypeError(f"table {key}: 4-byte elements expected, got {flat.dtype}")
                tables[top: top + flat.size] = flat.view(np.int32)
                top += flat.size
            d[f] = at
        d["tmp_off"] = tmp_top if p["tmp_bytes"] else 0
        tmp_top += _up(p["tmp_bytes"])
    return dict(block=block, images=images, tables=tables, tab_off=tab_off, table_elems=elems, tmp_bytes=tmp_top,
                n_tables=len(where))


# --------------------------------------------------------------------------------------------------
# launch
# --------------------------------------------------------------------------------------------------
def feed_batch_u8(src, images_dev_ptr: int, images_host: np.ndarray, tables_dev_ptr: int, table_elems: int, tmp, dst) -> int:
    """``wd_feed_batch_u8`` on the current stream.  ``src`` / ``tmp`` / ``dst``: device uint8 tensors (``tmp`` may be None),
    ``dst`` [B, H, W, 3]; ``images_host``: the structured descriptor array ``pack_batch`` returned (host), whose device
    copy lies at ``images_dev_ptr``; the table arena's device copy at ``tables_dev_ptr``.  Returns the kernels launched."""
    import torch
    if dst.dtype != torch.uint8 or dst.dim() != 4 or dst.shape[3] != 3 or not dst.is_cuda or not dst.is_contiguous():
        raise L.WedetectHipError("feed_batch_u8: dst must be a contiguous device uint8 [B, H, W, 3] tensor")
    if src.dtype != torch.uint8 or not src.is_cuda or (tmp is not None and (tmp.dtype != torch.uint8 or not tmp.is_cuda)):
        raise L.WedetectHipError("feed_batch_u8: src / tmp must be device uint8 tensors")
    b = int(dst.shape[0])
    if images_host.dtype != IMAGE_DTYPE or images_host.size != b or not images_host.flags.c_contiguous:
        raise L.WedetectHipError(f"feed_batch_u8: {b} descriptors expected")
    L.check(LIB.wd_feed_batch_u8(src.data_ptr(), src.numel(), images_dev_ptr, images_host.ctypes.data, b,
                                 tables_dev_ptr if table_elems else 0, int(table_elems), L.ptr(tmp), 0 if tmp is None else tmp.numel(),
                                 dst.data_ptr(), int(dst.shape[1]), int(dst.shape[2]), L.stream_ptr()), "wd_feed_batch_u8")
    return launches(images_host)


def launches(images_host: np.ndarray) -> int:
    """Kernel launches ``wd_feed_batch_u8`` issues for these descriptors."""
    return 2 if bool((images_host["mode"] == FEED_PILLOW).any()) else 1
