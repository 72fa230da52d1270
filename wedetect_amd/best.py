"""ctypes binding of the single-label ("best class") entry points (include/wedetect_hip_best.h, csrc/best.hip, the key epilogue
of csrc/split_gemm_p8.hip, the labeled form of the NMS kernel in csrc/postprocess.hip): the best class of every region row as a
64-bit key ``score bits << 32 | (0xFFFFFFFF - class)``, merged with an atomic maximum, so a bank may be scored in chunks.  Like
feed.py, tile.py, views.py and fold.py: a version and an export list of its own, the main ABI stays as it is."""
from __future__ import annotations

from . import lib as L
from .lib import f32, fp, i32, i64, vp

BEST_ABI_VERSION = 1
NMS_MMCV_AGNOSTIC = 3            # WD_NMS_MMCV_AGNOSTIC: mmcv.ops.batched_nms(..., class_agnostic=True)
FUSED_CHUNK = 1 << 20            # classes per wd_best_similarity_split launch (32-bit DMA offsets: n_cls * 768 * 4 < 2^32)
ROWS_CHUNK = 4096                # classes per materialised block on the other paths

SIGNATURES = {
    "wd_best_abi_version": (None, []),
    "wd_best_similarity_split": (None, [vp, i64, vp, f32, i32, i32, i32, i32, i32, fp, fp, vp, i32, vp, vp]),
    "wd_best_rows": (None, [vp, i32, i32, i32, i32, i32, vp, vp, vp]),
    "wd_best_unpack": (None, [vp, i64, vp, vp, vp]),
    "wd_nms_gather_labeled": (None, [vp, vp, vp, i32, vp, i32, vp, i32, vp, f32, i32, i32, i32, vp, i32, vp, vp, vp, vp, vp, vp, i32, vp, i64, vp]),
}
EXPORTS = tuple(SIGNATURES)
LIB = L.bind("best", BEST_ABI_VERSION, SIGNATURES)


def pack_key(score_bits, cls):
    """numpy restatement of the key: ``score_bits`` uint32 bit patterns of scores >= +0, ``cls`` class indices."""
    import numpy as np
    return (np.asarray(score_bits, np.uint64) << np.uint64(32)) | (np.uint64(0xFFFFFFFF) - np.asarray(cls, np.uint64))


def unpack_key(key):
    """(scores fp32, labels int32) of numpy uint64 keys; a key of 0 gives (0, -1)."""
    import numpy as np
    key = np.asarray(key, np.uint64)
    bits = (key >> np.uint64(32)).astype(np.uint32)
    lab = (np.uint64(0xFFFFFFFF) - (key & np.uint64(0xFFFFFFFF))).astype(np.int64)
    return np.where(key == 0, np.uint32(0), bits).view(np.float32), np.where(key == 0, -1, lab).astype(np.int32)


def best_similarity_split(e_split, rows, t_split, unscale, n_cls, dim, key, cls_offset=0, seg=None, range_flag=None, t_row=0) -> None:
    """``wd_best_similarity_split`` on the current stream; operands as :func:`lib.similarity_split`.  ``t_row``: the row of
    the split bank ``t_split`` at which this launch's chunk of ``n_cls`` rows begins (a multiple of eight unless the chunk ends
    the bank), ``cls_offset`` the class index of that row.  ``key``: int64 [rows]."""
    sr, e0, e1, sc, sb = L.seg_args(seg)
    L.check(LIB.wd_best_similarity_split(L.ptr(e_split), int(rows), L.bank_row_ptr(t_split, t_row, dim), float(unscale), int(n_cls),
                                         int(dim), sr, e0, e1, sc, sb, L.ptr(range_flag), int(cls_offset), L.ptr(key), L.stream_ptr()),
            "wd_best_similarity_split")


def best_rows(scores, n_img, rows_per_img, n_cls, ld, key, cls_offset=0, count=None) -> None:
    """``wd_best_rows`` on the current stream: merge the best column of every row of a [n_img * rows_per_img, ld] block."""
    L.check(LIB.wd_best_rows(L.ptr(scores), int(n_img), int(rows_per_img), int(n_cls), int(ld), int(cls_offset), L.ptr(count), L.ptr(key),
                             L.stream_ptr()), "wd_best_rows")


def best_unpack(key, rows, scores_out, labels_out) -> None:
    L.check(LIB.wd_best_unpack(L.ptr(key), int(rows), L.ptr(scores_out), L.ptr(labels_out), L.stream_ptr()), "wd_best_unpack")


def nms_gather_labeled(cand_idx, cand_score, cand_count, cand_stride, boxes, n_anchor, anchor_labels, n_label, meta, iou_thr, max_out,
                       embed, embed_dim, out_boxes, out_scores, out_labels, out_anchors, out_count, out_embed, batch,
                       nms_mode: int = L.NMS_VANILLA, mode_param: int = 0, workspace=None) -> None:
    """``wd_nms_gather_labeled`` on the current stream; ``iou_thr`` already rounded (:func:`lib.nms_threshold`)."""
    L.check(LIB.wd_nms_gather_labeled(L.ptr(cand_idx), L.ptr(cand_score), L.ptr(cand_count), int(cand_stride), L.ptr(boxes), int(n_anchor),
                                      L.ptr(anchor_labels), int(n_label), L.ptr(meta), float(iou_thr), int(max_out), int(nms_mode),
                                      int(mode_param), L.ptr(embed), int(embed_dim), L.ptr(out_boxes), L.ptr(out_scores), L.ptr(out_labels),
                                      L.ptr(out_anchors), L.ptr(out_count), L.ptr(out_embed), int(batch), L.ptr(workspace), L.nbytes(workspace),
                                      L.stream_ptr()), "wd_nms_gather_labeled")
