"""ctypes binding of the top-n entry points (include/wedetect_hip_topn.h, csrc/topn.hip, the top-n epilogue of
csrc/split_gemm_p8.hip): the ``n_top`` best classes of every region row as ``n_top`` 64-bit keys per row, each the best-class key
``score bits << 32 | (0xFFFFFFFF - class)`` (wedetect_amd/best.py), slot 0 being the best-class key itself.  Keys are merged by a
cascade of atomic maxima, so a bank may be scored in DISJOINT chunks in any order.  A version and an export list of its own, like
best.py and sparse.py: the main ABI stays as it is."""
from __future__ import annotations

import ctypes as C

from . import lib as L
from .best import _ptr, pack_key, unpack_key      # the key is the best-class key

TOPN_ABI_VERSION = 1
TOPN_MAX = 8                     # WD_TOPN_MAX
FUSED_CHUNK = 1 << 20            # classes per wd_topn_similarity_split launch (32-bit DMA offsets: n_cls * 768 * 4 < 2^32)
ROWS_CHUNK = 4096                # classes per materialised block on the other paths

EXPORTS = ("wd_topn_abi_version", "wd_topn_similarity_split", "wd_topn_rows", "wd_topn_unpack", "wd_topn_kept")


def _bind():
    lib = L.LIB
    for name in EXPORTS:
        if not hasattr(lib, name):
            raise L.WedetectHipMissing(f"{L.LIB_PATH} does not export {name}; rebuild (python -m wedetect_amd.build)")
    vp, i32, i64, f32 = C.c_void_p, C.c_int32, C.c_int64, C.c_float
    fp = C.POINTER(C.c_float)
    lib.wd_topn_abi_version.restype = C.c_int
    lib.wd_topn_similarity_split.argtypes = [vp, i64, vp, f32, i32, i32, i32, i32, i32, fp, fp, vp, vp, vp, i32, i32, vp, vp]
    lib.wd_topn_rows.argtypes = [vp, i32, i32, i32, i32, i32, vp, vp, vp, i32, vp, vp]
    lib.wd_topn_unpack.argtypes = [vp, i64, i32, i32, vp, vp, vp]
    lib.wd_topn_kept.argtypes = [vp, i32, i32, vp, vp, i32, i32, vp, vp, vp]
    if lib.wd_topn_abi_version() != TOPN_ABI_VERSION:
        raise L.WedetectHipMissing(f"topn ABI mismatch: library {lib.wd_topn_abi_version()} vs binding {TOPN_ABI_VERSION}; rebuild")
    return lib


LIB = _bind()


def check_n_top(n_top, lo: int = 1) -> int:
    """``n_top`` as an int in [lo, TOPN_MAX]; ValueError otherwise."""
    if isinstance(n_top, bool) or not isinstance(n_top, int) or not lo <= n_top <= TOPN_MAX:
        raise ValueError(f"top names: an int in {lo}..{TOPN_MAX} is supported, got {n_top!r}")
    return n_top


def pack(scores, labels):
    """numpy keys [rows, n] of (scores fp32 >= +0, labels int) lists; a label of -1 packs to the empty key 0."""
    import numpy as np
    scores, labels = np.ascontiguousarray(scores, np.float32), np.asarray(labels, np.int64)
    return np.where(labels < 0, np.uint64(0), pack_key(scores.view(np.uint32), np.maximum(labels, 0)))


def unpack(key):
    """(scores fp32, labels int32) of numpy uint64 keys of any shape; an empty key gives (0, -1)."""
    return unpack_key(key)


def topn_similarity_split(e_split, rows, t_split, unscale, n_cls, dim, n_top, key, cls_offset=0, seg=None, row_scale=None, row_bias=None,
                          range_flag=None, t_row=0) -> None:
    """``wd_topn_similarity_split`` on the current stream; operands as :func:`best.best_similarity_split`.  ``key``: int64
    [rows, n_top], cleared by the caller before the first producer of a step.  ``row_scale`` / ``row_bias`` fp32 [rows]: the
    per-region affine, exclusive with ``seg``."""
    sr, e0, e1 = (int(seg[0]), int(seg[1]), int(seg[2])) if seg is not None else (0, 0, 0)
    sc = (C.c_float * 3)(*[float(v) for v in (seg[3] if seg is not None else (1, 1, 1))])
    sb = (C.c_float * 3)(*[float(v) for v in (seg[4] if seg is not None else (0, 0, 0))])
    t_ptr = _ptr(t_split) + int(t_row) * ((int(dim) + 15) // 16 * 16) * 4
    L.check(LIB.wd_topn_similarity_split(_ptr(e_split), int(rows), t_ptr, float(unscale), int(n_cls), int(dim), sr, e0, e1, sc, sb,
                                         _ptr(row_scale), _ptr(row_bias), _ptr(range_flag), int(cls_offset), int(n_top), _ptr(key),
                                         L.stream_ptr()), "wd_topn_similarity_split")


def topn_rows(block, n_img, rows_per_img, n_cls, ld, n_top, key, cls_offset=0, count=None, row_scale=None, row_bias=None) -> None:
    """``wd_topn_rows`` on the current stream: merge the ``n_top`` best columns of every row of a [n_img * rows_per_img, ld] block
    (scores; raw logits where the row affine is given)."""
    L.check(LIB.wd_topn_rows(_ptr(block), int(n_img), int(rows_per_img), int(n_cls), int(ld), int(cls_offset), _ptr(count),
                             _ptr(row_scale), _ptr(row_bias), int(n_top), _ptr(key), L.stream_ptr()), "wd_topn_rows")


def topn_unpack(key, rows, n_top, slot, scores_out, labels_out) -> None:
    L.check(LIB.wd_topn_unpack(_ptr(key), int(rows), int(n_top), int(slot), _ptr(scores_out), _ptr(labels_out), L.stream_ptr()),
            "wd_topn_unpack")


def topn_kept(key, n_top, n_anchor, out_anchors, out_count, max_out, batch, top_scores, top_labels) -> None:
    L.check(LIB.wd_topn_kept(_ptr(key), int(n_top), int(n_anchor), _ptr(out_anchors), _ptr(out_count), int(max_out), int(batch),
                             _ptr(top_scores), _ptr(top_labels), L.stream_ptr()), "wd_topn_kept")
