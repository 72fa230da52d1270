"""numpy restatement of the "sparse scores" step (include/wedetect_hip_sparse.h) from a dense score block: the 64-bit keys, the
per-image candidate lists, and wd_sparse_select with its overflow / non-finite rules and the truncation at nms_pre."""
import numpy as np

STATUS_OK, STATUS_OVERFLOW, STATUS_NONFINITE = 0, 1, 2


def pack_key(scores, flat):
    """key = ~bits(score) << 32 | flat.  ``scores`` fp32 >= +0, ``flat`` flat (anchor, class) indices < 2^31."""
    bits = np.ascontiguousarray(scores, np.float32).view(np.uint32)
    return ((~bits).astype(np.uint64) << np.uint64(32)) | np.asarray(flat, np.uint64)


def unpack_key(key):
    key = np.asarray(key, np.uint64)
    return (~(key >> np.uint64(32)).astype(np.uint32)).view(np.float32), (key & np.uint64(0xFFFFFFFF)).astype(np.int64)


def image_list(scores, thr, n_cls_total=None, cls_offset=0, count=None):
    """The SORTED candidate keys of one image: ``scores`` [rows_per_img, n] fp32, column c is class cls_offset + c; flat =
    anchor * n_cls_total + class.  ``count``: only columns < count are read.  (The device lists hold the same keys in an
    order that depends on the schedule: compare sorted.)"""
    scores = np.ascontiguousarray(scores, np.float32)
    n = scores.shape[1]
    k = n if n_cls_total is None else int(n_cls_total)
    if count is not None:
        scores = scores[:, :max(0, min(int(count), n))]
    a, c = np.nonzero(scores > np.float32(thr))                  # strict fp32 comparison, as filter_scores_and_topk
    return np.sort(pack_key(scores[a, c], a.astype(np.int64) * k + cls_offset + c))


def lists(scores, n_img, thr, **kw):
    """Per-image sorted key lists and the state counters of a [n_img * rows_per_img, n] block."""
    blocks = np.ascontiguousarray(scores, np.float32).reshape(n_img, -1, scores.shape[-1])
    out = [image_list(blocks[b], thr, **kw) for b in range(n_img)]
    return out, np.asarray([v.shape[0] for v in out], np.int64)


def select(keys, n_seen, nonfinite, list_cap, nms_pre):
    """wd_sparse_select for one image: ``keys`` the image's list (any order; what fitted under list_cap), ``n_seen`` the counter.
    Returns (out_idx int32 [cap], out_score fp32 [cap], out_count, status), cap = the next power of two >= nms_pre."""
    cap = 1
    while cap < nms_pre:
        cap <<= 1
    idx, sc = np.full(cap, -1, np.int32), np.zeros(cap, np.float32)
    if nonfinite:
        return idx, sc, -1, STATUS_NONFINITE
    if n_seen > list_cap:
        return idx, sc, 0, STATUS_OVERFLOW
    k = np.sort(np.asarray(keys, np.uint64)[:n_seen])[:min(int(n_seen), int(nms_pre))]
    s, f = unpack_key(k)
    idx[:k.shape[0]], sc[:k.shape[0]] = f.astype(np.int32), s
    return idx, sc, int(k.shape[0]), STATUS_OK


def filter_topk(scores, thr, nms_pre, list_cap=1 << 20):
    """(scores, labels, anchors) of one image through keys -> select: what filter_scores_and_topk returns."""
    scores = np.ascontiguousarray(scores, np.float32)
    keys = image_list(scores, thr)
    idx, sc, n, status = select(keys, keys.shape[0], False, list_cap, nms_pre)
    assert status == STATUS_OK
    flat = idx[:n].astype(np.int64)
    return sc[:n], flat % scores.shape[1], flat // scores.shape[1]
