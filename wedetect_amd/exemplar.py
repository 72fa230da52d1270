"""ctypes binding of the exemplar-prompt entry points (include/wedetect_hip_exemplar.h, csrc/exemplar.hip): example boxes -> the
``m`` anchors that overlap each best (``wd_exemplar_assign``) and the selected anchors' region embeddings -> one unit bank row per
class (``wd_exemplar_pool``).  Between the two the kept-rows route of fold.py computes the embeddings (``wd_kept_rows_gather`` +
the three embedding GEMMs).  A version and an export list of its own, like topn.py: the main ABI stays as it is."""
from __future__ import annotations

from . import lib as L
from .lib import f32, i32, vp

EXEMPLAR_ABI_VERSION = 1
MAX_M = 8                        # WD_EXEMPLAR_MAX_M
MAX_EX = 64                      # WD_EXEMPLAR_MAX_EX

SIGNATURES = {
    "wd_exemplar_abi_version": (None, []),
    "wd_exemplar_assign": (None, [vp, i32, vp, vp, vp, i32, i32, i32, f32, vp, vp, vp, vp]),
    "wd_exemplar_pool": (None, [vp, i32, i32, i32, vp, vp, i32, vp, vp, i32, vp, vp, vp]),
}
EXPORTS = tuple(SIGNATURES)
LIB = L.bind("exemplar", EXEMPLAR_ABI_VERSION, SIGNATURES)


def check_m(m) -> int:
    """Anchors per example box as an int in 1..MAX_M; ValueError otherwise."""
    if isinstance(m, bool) or not isinstance(m, int) or not 1 <= m <= MAX_M:
        raise ValueError(f"anchors per example box: an int in 1..{MAX_M} is supported, got {m!r}")
    return m


def check_min_iou(min_iou) -> float:
    v = float(min_iou)
    if not 0.0 <= v < float("inf"):
        raise ValueError(f"min_iou: a finite value >= 0 is supported, got {min_iou!r}")
    return v


def exemplar_assign(boxes, n_anchor: int, ex_boxes, ex_count, meta, max_ex: int, batch: int, m: int, min_iou: float, sel_anchors,
                    sel_iou, sel_count) -> None:
    """``wd_exemplar_assign`` on the current stream: ``boxes`` fp32 [batch, n_anchor, 4] (network pixels), ``ex_boxes`` fp32
    [batch, max_ex, 4] (original-image pixels), ``ex_count`` int32 [batch], ``meta`` fp32 [batch, 8]; writes ``sel_anchors`` int32
    / ``sel_iou`` fp32 [batch, max_ex * m] and ``sel_count`` int32 [batch], whole."""
    L.check(LIB.wd_exemplar_assign(L.ptr(boxes), int(n_anchor), L.ptr(ex_boxes), L.ptr(ex_count), L.ptr(meta), int(max_ex), int(batch),
                                   int(m), float(min_iou), L.ptr(sel_anchors), L.ptr(sel_iou), L.ptr(sel_count), L.stream_ptr()),
            "wd_exemplar_assign")


def exemplar_pool(level_embed, dim: int, off1: int, off2: int, sel_anchors, sel_iou, n_slot: int, cls_off, cls_slot, n_cls: int,
                  bank, support) -> None:
    """``wd_exemplar_pool`` on the current stream: ``level_embed`` fp32 [3, n_slot, dim] (the three embedding GEMMs' outputs on the
    gathered rows), ``cls_off`` int32 [n_cls + 1] / ``cls_slot`` int32 [cls_off[-1]] the classes' slot lists; writes ``bank`` fp32
    [n_cls, dim] and ``support`` int32 [n_cls], whole."""
    L.check(LIB.wd_exemplar_pool(L.ptr(level_embed), int(dim), int(off1), int(off2), L.ptr(sel_anchors), L.ptr(sel_iou), int(n_slot),
                                 L.ptr(cls_off), L.ptr(cls_slot), int(n_cls), L.ptr(bank), L.ptr(support), L.stream_ptr()),
            "wd_exemplar_pool")
