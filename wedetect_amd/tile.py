"""ctypes binding of the tiled-inference entry points (include/wedetect_hip_tile.h, csrc/tile.hip): ``wd_tile_cut_u8`` cuts
an uploaded image into the [n_tile, th, tw, 3] tiles of a plan (wedetect_amd/tiling.py) in one launch, ``wd_tile_merge``
turns the stacked per-tile rows into the rows of the image.  Like feed.py: a version and an export list of its own, the main
ABI stays as it is."""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import lib as L
from .lib import f32, i32, i64, vp
from .tiling import TILE_DTYPE, TILE_FIELDS

TILE_ABI_VERSION = 1
MERGE_MAX_ROWS = 32768           # n_tile * max_in of one wd_tile_merge call
MERGE_MAX_OUT = 1024

SIGNATURES = {
    "wd_tile_abi_version": (None, []),
    "wd_tile_sizeof_tile": (i32, []),
    "wd_tile_cut_u8": (None, [vp, i32, i32, i64, vp, vp, i32, i32, i32, i32, i32, vp, vp]),
    "wd_tile_merge_workspace_bytes": (i64, [i32, i32]),
    "wd_tile_merge": (None, [vp, vp, vp, vp, vp, i32, i32, i32, f32, f32, i32, i32, vp, vp, vp, vp, vp, vp, i64, vp]),
}
EXPORTS = tuple(SIGNATURES)


class Tile(C.Structure):
    """Mirror of ``struct WdTile``."""
    _fields_ = [(n, C.c_int32) for n in TILE_FIELDS]


LIB = L.bind("tile", TILE_ABI_VERSION, SIGNATURES)
if not (LIB.wd_tile_sizeof_tile() == C.sizeof(Tile) == TILE_DTYPE.itemsize == 32):
    raise L.WedetectHipMissing("struct WdTile layout differs between the library and tile.Tile; rebuild")


def merge_workspace_bytes(n_tile: int, max_in: int) -> int:
    return int(LIB.wd_tile_merge_workspace_bytes(int(n_tile), int(max_in)))


def _plan_ok(plan_host: np.ndarray, n: int, what: str) -> None:
    if plan_host.dtype != TILE_DTYPE or plan_host.ndim != 1 or plan_host.size != n or not plan_host.flags.c_contiguous:
        raise L.WedetectHipError(f"{what}: {n} tile descriptors (tiling.TILE_DTYPE) expected")


def tile_cut_u8(img, plan_dev_ptr: int, plan_host: np.ndarray, dst, fill: int = 114, swap_rb: bool = False) -> None:
    """``wd_tile_cut_u8`` on the current stream.  ``img``: device uint8 [h, w, 3] whose rows may be strided (a view of a
    wider image); ``plan_host``: the descriptors, whose device copy lies at ``plan_dev_ptr``; ``dst``: contiguous device
    uint8 [n_tile, th, tw, 3]."""
    import torch
    if dst.dtype != torch.uint8 or dst.dim() != 4 or dst.shape[3] != 3 or not dst.is_cuda or not dst.is_contiguous():
        raise L.WedetectHipError("tile_cut_u8: dst must be a contiguous device uint8 [n_tile, th, tw, 3] tensor")
    if img.dtype != torch.uint8 or img.dim() != 3 or img.shape[2] != 3 or not img.is_cuda or img.stride(2) != 1 or img.stride(1) != 3:
        raise L.WedetectHipError("tile_cut_u8: img must be a device uint8 [h, w, 3] tensor with dense pixels")
    n = int(dst.shape[0])
    _plan_ok(plan_host, n, "tile_cut_u8")
    L.check(LIB.wd_tile_cut_u8(img.data_ptr(), int(img.shape[0]), int(img.shape[1]), int(img.stride(0)), plan_dev_ptr,
                               plan_host.ctypes.data, n, int(dst.shape[1]), int(dst.shape[2]), int(fill), int(bool(swap_rb)),
                               dst.data_ptr(), L.stream_ptr()), "wd_tile_cut_u8")


def tile_merge(boxes, scores, labels, counts, plan_dev_ptr: int, n_tile: int, max_in: int, n_cls: int, edge_margin: float,
               iou_thr: float, split_thr: int, max_out: int, out_boxes, out_scores, out_labels, out_src, out_count, workspace) -> None:
    """``wd_tile_merge`` on the current stream; ``iou_thr`` is rounded as mmcv's ``float iou_threshold`` is
    (``lib.nms_threshold``)."""
    L.check(LIB.wd_tile_merge(boxes.data_ptr(), scores.data_ptr(), labels.data_ptr(), counts.data_ptr(), plan_dev_ptr, int(n_tile),
                              int(max_in), int(n_cls), float(edge_margin), L.nms_threshold(iou_thr, L.NMS_MMCV), int(split_thr),
                              int(max_out), out_boxes.data_ptr(), out_scores.data_ptr(), out_labels.data_ptr(), out_src.data_ptr(),
                              out_count.data_ptr(), workspace.data_ptr(), L.nbytes(workspace), L.stream_ptr()), "wd_tile_merge")
