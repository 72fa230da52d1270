"""ctypes binding of the "sparse scores" entry points (include/wedetect_hip_sparse.h, csrc/sparse.hip, the candidate epilogue of
csrc/split_gemm_p8.hip): the multi-label step without the score tensor.  The (anchor, class) pairs with ``score > thr`` are appended
to a per-image list of 64-bit keys ``~score bits << 32 | flat index`` — the key ``wd_topk_candidates`` sorts by — and
``wd_sparse_select`` sorts a list into the buffers ``wd_nms_gather`` reads.  Like best.py: a version and an export list of its own,
the main ABI stays as it is."""
from __future__ import annotations

import ctypes as C

from . import lib as L

SPARSE_ABI_VERSION = 1
STATUS_OK, STATUS_OVERFLOW, STATUS_NONFINITE = 0, 1, 2
FUSED_CHUNK = 1 << 20            # classes per wd_sparse_similarity_split launch (32-bit DMA offsets: n_cls * 768 * 4 < 2^32)
ROWS_CHUNK = 4096                # classes per materialised block on the other paths
MAX_LIST_CAP = 1 << 20

EXPORTS = ("wd_sparse_abi_version", "wd_sparse_similarity_split", "wd_sparse_rows", "wd_sparse_select")


def _bind():
    lib = L.LIB
    for name in EXPORTS:
        if not hasattr(lib, name):
            raise L.WedetectHipMissing(f"{L.LIB_PATH} does not export {name}; rebuild (python -m wedetect_amd.build)")
    vp, i32, i64, f32 = C.c_void_p, C.c_int32, C.c_int64, C.c_float
    fp = C.POINTER(C.c_float)
    lib.wd_sparse_abi_version.restype = C.c_int
    lib.wd_sparse_similarity_split.argtypes = [vp, i64, vp, f32, i32, i32, i32, i32, i32, fp, fp, vp, i32, i32, i32, f32, vp, i32, vp, vp]
    lib.wd_sparse_rows.argtypes = [vp, i32, i32, i32, i32, i32, vp, i32, f32, vp, i32, vp, vp]
    lib.wd_sparse_select.argtypes = [vp, i32, vp, i32, i32, vp, vp, vp, vp, vp]
    if lib.wd_sparse_abi_version() != SPARSE_ABI_VERSION:
        raise L.WedetectHipMissing(f"sparse ABI mismatch: library {lib.wd_sparse_abi_version()} vs binding {SPARSE_ABI_VERSION}; rebuild")
    return lib


LIB = _bind()


def _ptr(t) -> int:
    """A tensor's address, an address given as an int, or 0."""
    return 0 if t is None else (int(t) if isinstance(t, int) else t.data_ptr())


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
    sr, e0, e1 = (int(seg[0]), int(seg[1]), int(seg[2])) if seg is not None else (0, 0, 0)
    sc = (C.c_float * 3)(*[float(v) for v in (seg[3] if seg is not None else (1, 1, 1))])
    sb = (C.c_float * 3)(*[float(v) for v in (seg[4] if seg is not None else (0, 0, 0))])
    t_ptr = _ptr(t_split) + int(t_row) * ((int(dim) + 15) // 16 * 16) * 4
    L.check(LIB.wd_sparse_similarity_split(_ptr(e_split), int(rows), t_ptr, float(unscale), int(n_cls), int(dim), sr, e0, e1, sc, sb,
                                           _ptr(range_flag), int(cls_offset), int(rows_per_img), int(n_cls_total), float(thr),
                                           _ptr(list_), int(list_cap), _ptr(state), L.stream_ptr()), "wd_sparse_similarity_split")


def sparse_rows(scores, n_img, rows_per_img, n_cls, ld, n_cls_total, thr, list_, list_cap, state, cls_offset=0, count=None) -> None:
    """``wd_sparse_rows`` on the current stream: append the candidates of a [n_img * rows_per_img, ld] score block."""
    L.check(LIB.wd_sparse_rows(_ptr(scores), int(n_img), int(rows_per_img), int(n_cls), int(ld), int(cls_offset), _ptr(count),
                               int(n_cls_total), float(thr), _ptr(list_), int(list_cap), _ptr(state), L.stream_ptr()), "wd_sparse_rows")


def sparse_select(list_, list_cap, state, batch, nms_pre, out_idx, out_score, out_count, status) -> None:
    """``wd_sparse_select`` on the current stream: sorts the lists in place and writes the candidate buffers of
    ``wd_topk_candidates`` plus ``status`` int32 [batch]."""
    L.check(LIB.wd_sparse_select(_ptr(list_), int(list_cap), _ptr(state), int(batch), int(nms_pre), _ptr(out_idx), _ptr(out_score),
                                 _ptr(out_count), _ptr(status), L.stream_ptr()), "wd_sparse_select")
