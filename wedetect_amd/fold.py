"""ctypes binding of the folded-text-bank entry points (include/wedetect_hip_fold.h; csrc/fold.hip, csrc/split_gemm.hip):
``wd_fold_similarity`` scores one head level from the level's c2 rows with the bank folded into the embedding conv,
``wd_kept_rows_gather`` / ``wd_kept_rows_select`` move the rows the post-process kept into and out of the three embedding
GEMMs that compute their 768-d embeddings, ``wd_kept_rows_reorder`` gives the kept rows the scores of the unfolded similarity
GEMM (run on those embeddings) and the order they imply.  Like feed.py, tile.py and views.py: a version and an export list of its own, the
main ABI stays as it is."""
from __future__ import annotations

import ctypes as C

from . import lib as L
from .lib import f32, i32, vp

FOLD_ABI_VERSION = 1

SIGNATURES = {
    "wd_fold_abi_version": (None, []),
    "wd_fold_similarity": (None, [C.POINTER(L.ConvGemm), vp, f32, vp, vp]),
    "wd_kept_rows_gather": (None, [vp, vp, vp, i32, i32, i32, i32, vp, vp, i32, i32, vp, vp]),
    "wd_kept_rows_select": (None, [vp, i32, i32, i32, vp, vp, vp, i32, i32, vp, vp]),
    "wd_kept_rows_reorder": (None, [vp, i32, i32, i32, i32, vp, vp, vp, vp, vp, i32, i32, vp, vp]),
}
EXPORTS = tuple(SIGNATURES)
LIB = L.bind("fold", FOLD_ABI_VERSION, SIGNATURES)


def fold_similarity(c2_split, w_split, unscale: float, unscale_dev, bias, out, *, batch: int, rows: int, cin: int, n: int,
                    c_batch_stride: int, out_scale: float, out_bias: float, sigmoid: bool = True, range_flag=None) -> None:
    """One level of the folded similarity on the current stream: ``out`` (a view of the [B, anchors, K] scores that starts at
    the level's first row) <- sigmoid((<c2, Wf> * unscale * unscale_dev + bias) * out_scale + out_bias) for the ``rows``
    anchors per image of the level.  ``c2_split``: the level's pre-split c2 rows [batch * rows, cin]; ``w_split``:
    ``wd_split_weights_padded`` of the [n, cin] folded weights; ``bias``: round_up(n, 8) floats."""
    p = L.ConvGemm(a=L.ptr(c2_split), w=0, bias=L.ptr(bias), res=0, c=L.ptr(out), batch=batch, hin=1, win=rows, cin=cin, lda=cin,
                   kh=1, kw=1, stride=1, pad=0, hout=1, wout=rows, m=batch * rows, n=n, k=cin, ldc=n, ldres=0, act=L.ACT_NONE,
                   out_mode=L.OUT_ROWS, res_alpha=1.0, out_scale=out_scale, out_bias=out_bias, sigmoid=int(bool(sigmoid)),
                   c_batch_stride=c_batch_stride, range_flag=L.ptr(range_flag), c2=0, ldc2=0, a_scale=1.0, c_split_scale=1.0,
                   ln_stats=0, ln_u=0)
    L.check(LIB.wd_fold_similarity(C.byref(p), L.ptr(w_split), float(unscale), L.ptr(unscale_dev), L.stream_ptr()),
            "wd_fold_similarity")


def kept_rows_gather(c2, rows, row_floats: int, out_anchors, out_count, max_out: int, batch: int, gathered) -> None:
    """``wd_kept_rows_gather`` on the current stream; ``c2`` / ``rows``: the three levels' buffers and anchors per image."""
    L.check(LIB.wd_kept_rows_gather(L.ptr(c2[0]), L.ptr(c2[1]), L.ptr(c2[2]), int(rows[0]), int(rows[1]), int(rows[2]),
                                    int(row_floats), L.ptr(out_anchors), L.ptr(out_count), int(max_out), int(batch), L.ptr(gathered),
                                    L.stream_ptr()), "wd_kept_rows_gather")


def kept_rows_select(level_embed, dim: int, off1: int, off2: int, out_anchors, out_count, max_out: int, batch: int,
                     out_embed, perm=None) -> None:
    """``wd_kept_rows_select`` on the current stream; ``perm``: what :func:`kept_rows_reorder` wrote, or None."""
    L.check(LIB.wd_kept_rows_select(L.ptr(level_embed), int(dim), int(off1), int(off2), L.ptr(out_anchors), L.ptr(out_count),
                                    L.ptr(perm), int(max_out), int(batch), L.ptr(out_embed), L.stream_ptr()), "wd_kept_rows_select")


def kept_rows_reorder(level_scores, k: int, n_anchor: int, off1: int, off2: int, out_boxes, out_scores, out_labels, out_anchors,
                      out_count, max_out: int, batch: int, perm) -> None:
    """``wd_kept_rows_reorder`` on the current stream: the kept rows get the unfolded GEMM's scores (``level_scores``
    [3, batch * max_out, k]) and their order, in place; ``perm`` int32 [batch, max_out] receives where each row came from."""
    L.check(LIB.wd_kept_rows_reorder(L.ptr(level_scores), int(k), int(n_anchor), int(off1), int(off2), L.ptr(out_boxes),
                                     L.ptr(out_scores), L.ptr(out_labels), L.ptr(out_anchors), L.ptr(out_count), int(max_out),
                                     int(batch), L.ptr(perm), L.stream_ptr()), "wd_kept_rows_reorder")
