"""ctypes binding of the top-n entry points (include/wedetect_hip_topn.h, csrc/topn.hip, the top-n epilogue of
csrc/split_gemm_p8.hip): the ``n_top`` best classes of every region row as ``n_top`` 64-bit keys per row, each the best-class key
``score bits << 32 | (0xFFFFFFFF - class)`` (wedetect_amd/best.py), slot 0 being the best-class key itself.  Keys are merged by a
cascade of atomic maxima, so a bank may be scored in DISJOINT chunks in any order.  A version and an export list of its own, like
best.py and sparse.py: the main ABI stays as it is."""
from __future__ import annotations

from . import lib as L
from .best import pack_key, unpack_key            # the key is the best-class key
from .lib import f32, fp, i32, i64, vp

TOPN_ABI_VERSION = 1
TOPN_MAX = 8                     # WD_TOPN_MAX
FUSED_CHUNK = 1 << 20            # classes per wd_topn_similarity_split launch (32-bit DMA offsets: n_cls * 768 * 4 < 2^32)
ROWS_CHUNK = 4096                # classes per materialised block on the other paths

SIGNATURES = {
    "wd_topn_abi_version": (None, []),
    "wd_topn_similarity_split": (None, [vp, i64, vp, f32, i32, i32, i32, i32, i32, fp, fp, vp, vp, vp, i32, i32, vp, vp]),
    "wd_topn_rows": (None, [vp, i32, i32, i32, i32, i32, vp, vp, vp, i32, vp, vp]),
    "wd_topn_unpack": (None, [vp, i64, i32, i32, vp, vp, vp]),
    "wd_topn_kept": (None, [vp, i32, i32, vp, vp, i32, i32, vp, vp, vp]),
}
EXPORTS = tuple(SIGNATURES)
LIB = L.bind("topn", TOPN_ABI_VERSION, SIGNATURES)


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
    sr, e0, e1, sc, sb = L.seg_args(seg)
    L.check(LIB.wd_topn_similarity_split(L.ptr(e_split), int(rows), L.bank_row_ptr(t_split, t_row, dim), float(unscale), int(n_cls),
                                         int(dim), sr, e0, e1, sc, sb, L.ptr(row_scale), L.ptr(row_bias), L.ptr(range_flag),
                                         int(cls_offset), int(n_top), L.ptr(key), L.stream_ptr()), "wd_topn_similarity_split")


def topn_rows(block, n_img, rows_per_img, n_cls, ld, n_top, key, cls_offset=0, count=None, row_scale=None, row_bias=None) -> None:
    """``wd_topn_rows`` on the current stream: merge the ``n_top`` best columns of every row of a [n_img * rows_per_img, ld] block
    (scores; raw logits where the row affine is given)."""
    L.check(LIB.wd_topn_rows(L.ptr(block), int(n_img), int(rows_per_img), int(n_cls), int(ld), int(cls_offset), L.ptr(count),
                             L.ptr(row_scale), L.ptr(row_bias), int(n_top), L.ptr(key), L.stream_ptr()), "wd_topn_rows")


def topn_unpack(key, rows, n_top, slot, scores_out, labels_out) -> None:
    L.check(LIB.wd_topn_unpack(L.ptr(key), int(rows), int(n_top), int(slot), L.ptr(scores_out), L.ptr(labels_out), L.stream_ptr()),
            "wd_topn_unpack")


def topn_kept(key, n_top, n_anchor, out_anchors, out_count, max_out, batch, top_scores, top_labels) -> None:
    L.check(LIB.wd_topn_kept(L.ptr(key), int(n_top), int(n_anchor), L.ptr(out_anchors), L.ptr(out_count), int(max_out), int(batch),
                             L.ptr(top_scores), L.ptr(top_labels), L.stream_ptr()), "wd_topn_kept")
