"""ctypes binding of the test-time-augmentation entry points (include/wedetect_hip_views.h, csrc/views.hip): ``wd_flip_u8``
flips a batch of [n, h, w, 3] images in one launch, ``wd_views_merge`` turns the stacked per-view rows of every image into the
rows of that image.  Like feed.py and tile.py: a version and an export list of its own, the main ABI stays as it is."""
from __future__ import annotations

from . import lib as L
from .lib import f32, i32, i64, vp

VIEWS_ABI_VERSION = 1
MERGE_MAX_VIEWS = 8
MERGE_MAX_ROWS = 4096            # n_view * max_in of one image
MERGE_MAX_OUT = 1024
FLIP_CODES = {None: 0, "horizontal": 1, "vertical": 2, "diagonal": 3}      # mmcv imflip directions -> WD_FLIP_*

SIGNATURES = {
    "wd_views_abi_version": (None, []),
    "wd_flip_u8": (None, [vp, vp, i32, i32, i32, i32, vp]),
    "wd_views_merge_workspace_bytes": (i64, [i32, i32, i32]),
    "wd_views_merge": (None, [vp, vp, vp, vp, vp, vp, i32, i32, i32, i32, f32, i32, i32, vp, vp, vp, vp, vp, vp, i64, vp]),
}
EXPORTS = tuple(SIGNATURES)
LIB = L.bind("views", VIEWS_ABI_VERSION, SIGNATURES)


def merge_workspace_bytes(n_view: int, batch: int, max_in: int) -> int:
    return int(LIB.wd_views_merge_workspace_bytes(int(n_view), int(batch), int(max_in)))


def flip_u8(src, dst, direction) -> None:
    """``wd_flip_u8`` on the current stream.  ``src`` / ``dst``: contiguous device uint8 [h, w, 3] or [n, h, w, 3] of one shape;
    ``direction``: 'horizontal' / 'vertical' / 'diagonal' or the code 1 .. 3."""
    import torch
    code = FLIP_CODES.get(direction, direction) if isinstance(direction, (str, type(None))) else int(direction)
    if code not in (1, 2, 3):
        raise L.WedetectHipError(f"flip_u8: direction {direction!r} (horizontal / vertical / diagonal)")
    for t in (src, dst):
        if t.dtype != torch.uint8 or t.dim() not in (3, 4) or t.shape[-1] != 3 or not t.is_cuda or not t.is_contiguous():
            raise L.WedetectHipError("flip_u8: contiguous device uint8 [n, h, w, 3] (or [h, w, 3]) tensors are required")
    if src.shape != dst.shape:
        raise L.WedetectHipError("flip_u8: src and dst differ in shape")
    n = int(src.shape[0]) if src.dim() == 4 else 1
    L.check(LIB.wd_flip_u8(src.data_ptr(), dst.data_ptr(), n, int(src.shape[-3]), int(src.shape[-2]), code, L.stream_ptr()), "wd_flip_u8")


def views_merge(boxes, scores, labels, counts, view_flip, img_wh, n_view: int, batch: int, max_in: int, n_cls: int, iou_thr: float,
                split_thr: int, max_out: int, out_boxes, out_scores, out_labels, out_src, out_count, workspace) -> None:
    """``wd_views_merge`` on the current stream; ``iou_thr`` is rounded as mmcv's ``float iou_threshold`` is
    (``lib.nms_threshold``)."""
    L.check(LIB.wd_views_merge(boxes.data_ptr(), scores.data_ptr(), labels.data_ptr(), counts.data_ptr(), view_flip.data_ptr(),
                               img_wh.data_ptr(), int(n_view), int(batch), int(max_in), int(n_cls), L.nms_threshold(iou_thr, L.NMS_MMCV),
                               int(split_thr), int(max_out), out_boxes.data_ptr(), out_scores.data_ptr(), out_labels.data_ptr(),
                               out_src.data_ptr(), out_count.data_ptr(), workspace.data_ptr(), L.nbytes(workspace),
                               L.stream_ptr()), "wd_views_merge")
