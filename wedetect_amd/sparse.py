"""ctypes binding of the "sparse scores" entry points (include/wedetect_hip_sparse.h, csrc/sparse.hip, the candidate epilogue of
csrc/split_gemm_p8.hip): the multi-label step without the score tensor.  The (anchor, class) pairs with ``score > thr`` are appended
to a per-image list of 64-bit keys ``~score bits << 32 | flat index`` — the key ``wd_topk_candidates`` sorts by — and
``wd_sparse_select`` sorts a list into the buffers ``wd_nms_gather`` reads.  Like best.py: a version and an export list of its own,
the main ABI stays as it is."""
from __future__ import annotations

from . import lib as L
from .lib import f32, fp, i32, i64, vp

SPARSE_ABI_VERSION = 1
STATUS_OK, STATUS_OVERFLOW, STATUS_NONFINITE = 0, 1, 2
FUSED_CHUNK = 1 << 20            # classes per wd_sparse_similarity_split launch (32-bit DMA offsets: n_cls * 768 * 4 < 2^32)
ROWS_CHUNK = 4096                # classes per materialised block on the other paths
MAX_LIST_CAP = 1 << 20

SIGNATURES = {
    "wd_sparse_abi_version": (None, []),
    "wd_sparse_similarity_split": (None, [vp, i64, vp, f32, i32, i32, i32, i32, i32, fp, fp, vp, i32, i32, i32, f32, vp, i32, vp, vp]),
    "wd_sparse_rows": (None, [vp, i32, i32, i32, i32, i32, vp, i32, f32, vp, i32, vp, vp]),
    "wd_sparse_select": (None, [vp, i32, vp, i32, i32, vp, vp, vp, vp, vp]),
}
EXPORTS = tuple(SIGNATURES)
LIB = L.bind("sparse", SPARSE_ABI_VERSION, SIGNATURES)


def list_capacity(sparse_cap: int, nms_pre: int) -> int:
    """The list capacity for a requested ``sparse_cap``: the next power of two, at least ``wd_topk_capacity(nms_pre)``."""
    cap = max(int(sparse_cap), int(L.LIB.wd_topk_capacity(int(nms_pre))), 1)
    cap = 1 << (cap - 1).bit_length()
    if cap > MAX_LIST_CAP:
        raise ValueError(f"sparse_cap {sparse_cap} (nms_pre {nms_pre}) exceeds {MAX_LIST_CAP} list entries per image")
    return cap


def sparse_similarity_split(e_split, rows, t_split, unscale, n_cls, dim, rows_per_img, n_cls_total, thr, list_, list_cap, state,
                            cls_offset=0, seg=None, range_flag=None, t_row=0) -> None:
    """``wd_sparse_similarity_split`` on the current stream; operands as :func:`best.best_similarity_split`.  ``list_``: int64
    [batch, list_cap]; ``state``: int32 [batch, 2], zeroed by the caller before the first producer of a step."""
    sr, e0, e1, sc, sb = L.seg_args(seg)
    L.check(LIB.wd_sparse_similarity_split(L.ptr(e_split), int(rows), L.bank_row_ptr(t_split, t_row, dim), float(unscale), int(n_cls),
                                           int(dim), sr, e0, e1, sc, sb, L.ptr(range_flag), int(cls_offset), int(rows_per_img), int(n_cls_total), float(thr),
                                           L.ptr(list_), int(list_cap), L.ptr(state), L.stream_ptr()), "wd_sparse_similarity_split")


def sparse_rows(scores, n_img, rows_per_img, n_cls, ld, n_cls_total, thr, list_, list_cap, state, cls_offset=0, count=None) -> None:
    """``wd_sparse_rows`` on the current stream: append the candidates of a [n_img * rows_per_img, ld] score block."""
    L.check(LIB.wd_sparse_rows(L.ptr(scores), int(n_img), int(rows_per_img), int(n_cls), int(ld), int(cls_offset), L.ptr(count),
                               int(n_cls_total), float(thr), L.ptr(list_), int(list_cap), L.ptr(state), L.stream_ptr()), "wd_sparse_rows")


def sparse_select(list_, list_cap, state, batch, nms_pre, out_idx, out_score, out_count, status) -> None:
    """``wd_sparse_select`` on the current stream: sorts the lists in place and writes the candidate buffers of
    ``wd_topk_candidates`` plus ``status`` int32 [batch]."""
    L.check(LIB.wd_sparse_select(L.ptr(list_), int(list_cap), L.ptr(state), int(batch), int(nms_pre), L.ptr(out_idx), L.ptr(out_score),
                                 L.ptr(out_count), L.ptr(status), L.stream_ptr()), "wd_sparse_select")
