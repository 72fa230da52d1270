"""ctypes binding of the exemplar-prompt entry points (include/wedetect_hip_exemplar.h, csrc/exemplar.hip): example boxes -> the
``m`` anchors that overlap each best (``wd_exemplar_assign``) and the selected anchors' region embeddings -> one unit bank row per
class (``wd_exemplar_pool``).  Between the two the kept-rows route of fold.py computes the embeddings (``wd_kept_rows_gather`` +
the three embedding GEMMs).  A version and an export list of its own, like topn.py: the main ABI stays as it is."""
from __future__ import annotations

import ctypes as C

from . import lib as L

EXEMPLAR_ABI_VERSION = 1
MAX_M = 8                        # WD_EXEMPLAR_MAX_M
MAX_EX = 64                      # WD_EXEMPLAR_MAX_EX

EXPORTS = ("wd_exemplar_abi_version", "wd_exemplar_assign", "wd_exemplar_pool")


def _bind():
    lib = L.LIB
    for name in EXPORTS:
        if not hasattr(lib, name):
            raise L.WedetectHipMissing(f"{L.LIB_PATH} does not export {name}; rebuild (python -m wedetect_amd.build)")
    vp, i32, f32 = C.c_void_p, C.c_int32, C.c_float
    lib.wd_exemplar_abi_version.restype = C.c_int
    lib.wd_exemplar_assign.argtypes = [vp, i32, vp, vp, vp, i32, i32, i32, f32, vp, vp, vp, vp]
    lib.wd_exemplar_pool.argtypes = [vp, i32, i32, i32, vp, vp, i32, vp, vp, i32, vp, vp, vp]
    if lib.wd_exemplar_abi_version() != EXEMPLAR_ABI_VERSION:
        raise L.WedetectHipMissing(f"exemplar ABI mismatch: library {lib.wd_exemplar_abi_version()} vs binding {EXEMPLAR_ABI_VERSION}; rebuild")
    return lib


LIB = _bind()


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
    L.check(LIB.wd_exemplar_assign(L._p(boxes), int(n_anchor), L._p(ex_boxes), L._p(ex_count), L._p(meta), int(max_ex), int(batch),
                                   int(m), float(min_iou), L._p(sel_anchors), L._p(sel_iou), L._p(sel_count), L.stream_ptr()),
            "wd_exemplar_assign")


def exemplar_pool(level_embed, dim: int, off1: int, off2: int, sel_anchors, sel_iou, n_slot: int, cls_off, cls_slot, n_cls: int,
                  bank, support) -> None:
    """``wd_exemplar_pool`` on the current stream: ``level_embed`` fp32 [3, n_slot, dim] (the three embedding GEMMs' outputs on the
    gathered rows), ``cls_off`` int32 [n_cls + 1] / ``cls_slot`` int32 [cls_off[-1]] the classes' slot lists; writes ``bank`` fp32
    [n_cls, dim] and ``support`` int32 [n_cls], whole."""
    L.check(LIB.wd_exemplar_pool(L._p(level_embed), int(dim), int(off1), int(off2), L._p(sel_anchors), L._p(sel_iou), int(n_slot),
                                 L._p(cls_off), L._p(cls_slot), int(n_cls), L._p(bank), L._p(support), L.stream_ptr()),
            "wd_exemplar_pool")
