"""The device entry points of include/wedetect_hip_sparse.h (GPU): the fused similarity + candidate append against the
materialising launch (the SET of keys must equal wd_sparse_rows over its output and numpy, bit for bit), wd_sparse_select
against wd_topk_candidates on that output, chunks, ties, empty / overflowing lists, one image overflowing, the non-finite
guard, wd_sparse_rows with per-image counts, argument errors.

Shapes (those of tests/test_gpu_best_kernels.py): 2 x 525 rows — a row tile and a 32-row group straddle both images, waves
straddle the level boundaries at 400 and 500 — dim 768, banks of 257 / 1203 / 4100 rows (a ragged last tile, more than one
group of eight column tiles).  Every threshold is an order statistic of the dense output, asserted on it before the sparse
launch."""
import numpy as np
import pytest
import torch

import tests.sparse_hazards  # noqa: F401
from tests import sparse_ref as R
from tests.test_gpu_best_kernels import DIM, ENDS, ES_SCALE, NTOT, SEG, _operands
from tests.test_gpu_split import _rand, _to_split_padded

pytestmark = pytest.mark.gpu

POISON = 0x5555555555555555
POISON32 = 0x55555555
B = 2
_CACHE = {}


def _dense(k_cls, seg=SEG, img1_scale=None):
    """Operands and the dense wd_similarity_split output, computed once per case and left unchanged."""
    from wedetect_amd import lib as L
    tag = (k_cls, seg[3], img1_scale)
    if tag not in _CACHE:
        rows = B * NTOT
        e, t = _operands(B, k_cls, False)
        if img1_scale is not None:
            e = e.clone()
            e[NTOT:] *= img1_scale
        es, ts = _to_split_padded(e, ES_SCALE), L.split_weights(t)
        flag = torch.zeros(1, dtype=torch.int32, device="cuda")
        out = torch.empty(rows, k_cls, device="cuda")
        L.similarity_split(es, rows, ts[0], ts[1] / ES_SCALE, out, k_cls, DIM, k_cls, seg=seg, sigmoid=True, range_flag=flag)
        torch.cuda.synchronize()
        assert int(flag) == 0
        _CACHE[tag] = dict(es=es, ts=ts, out=out, out_np=out.cpu().numpy(), rows=rows, k=k_cls, seg=seg)
    return _CACHE[tag]


def _kth_largest(a, k):
    """The k-th largest value of ``a`` (k >= 1): ``a > it`` holds for fewer than k elements."""
    flat = np.asarray(a, np.float32).reshape(-1)
    return float(np.partition(flat, flat.shape[0] - k)[flat.shape[0] - k])


def _counts(c, thr):
    return [int((c["out_np"][b * NTOT:(b + 1) * NTOT] > np.float32(thr)).sum()) for b in range(B)]


def _buffers(list_cap, b=B):
    """(list, state, raw list buffer, raw state buffer): poisoned, with four poison words behind each."""
    raw = torch.full((b * list_cap + 4,), POISON, dtype=torch.int64, device="cuda")
    sraw = torch.full((2 * b + 4,), POISON32, dtype=torch.int32, device="cuda")
    sraw[:2 * b] = 0
    return raw[:b * list_cap].view(b, list_cap), sraw[:2 * b].view(b, 2), raw, sraw


def _fused(c, thr, lst, list_cap, state, cuts=None, flag=None, k_total=None):
    from wedetect_amd import sparse as SP
    k = c["k"]
    for a, z in (cuts or [(0, k)]):
        SP.sparse_similarity_split(c["es"], c["rows"], c["ts"][0], c["ts"][1] / ES_SCALE, z - a, DIM, NTOT, k_total or k, thr, lst,
                                   list_cap, state, cls_offset=a, seg=c["seg"], range_flag=flag, t_row=a)


def _sorted_lists(lst, state, list_cap):
    """Per-image numpy uint64 keys of the device lists, sorted; asserts the poison behind the counters' ends."""
    torch.cuda.synchronize()
    seen = state[:, 0].cpu().numpy()
    host = lst.cpu().numpy().view(np.uint64)
    out = []
    for b in range(lst.shape[0]):
        n = min(int(seen[b]), list_cap)
        assert bool((host[b, n:] == np.uint64(POISON)).all()), "list slots past the counter were written"
        out.append(np.sort(host[b, :n]))
    return out, seen


def _same(a, b):
    return torch.equal(torch.from_numpy(np.ascontiguousarray(a).view(np.int64)), torch.from_numpy(np.ascontiguousarray(b).view(np.int64)))


def _select(lst, list_cap, state, nms_pre, b=B):
    from wedetect_amd import lib as L
    from wedetect_amd import sparse as SP
    cap = L.topk_capacity(nms_pre)
    idx = torch.full((b * cap + 4,), 7, dtype=torch.int32, device="cuda")
    sc = torch.full((b * cap + 4,), 7.0, device="cuda")
    cnt = torch.full((b + 4,), 7, dtype=torch.int32, device="cuda")
    status = torch.full((b + 4,), 7, dtype=torch.int32, device="cuda")
    SP.sparse_select(lst, list_cap, state, b, nms_pre, idx, sc, cnt, status)
    torch.cuda.synchronize()
    for t, n in ((idx, b * cap), (cnt, b), (status, b)):
        assert bool((t[n:] == 7).all())
    assert bool((sc[b * cap:] == 7.0).all())
    return idx[:b * cap].view(b, cap), sc[:b * cap].view(b, cap), cnt[:b], status[:b]


def _dense_topk(out, n_per_img, thr, nms_pre, b=B):
    from wedetect_amd import lib as L
    cap = L.topk_capacity(nms_pre)
    idx = torch.full((b, cap), 7, dtype=torch.int32, device="cuda")
    sc = torch.full((b, cap), 7.0, device="cuda")
    cnt = torch.full((b,), 7, dtype=torch.int32, device="cuda")
    ws = torch.empty(L.topk_workspace_bytes(b, n_per_img, nms_pre) + 256, dtype=torch.uint8, device="cuda")
    ws = ws[(-ws.data_ptr()) % 256:]
    L.topk_candidates(out, b, n_per_img, thr, nms_pre, idx, sc, cnt, ws)
    torch.cuda.synchronize()
    return idx, sc, cnt


def _assert_select_equals_dense(c, thr, lst, list_cap, state, nms_pre, images=(0, 1)):
    idx, sc, cnt, status = _select(lst.clone(), list_cap, state, nms_pre)
    didx, dsc, dcnt = _dense_topk(c["out"], NTOT * c["k"], thr, nms_pre)
    for b in images:
        assert int(status[b]) == 0
        assert torch.equal(idx[b], didx[b]) and torch.equal(sc[b], dsc[b]) and torch.equal(cnt[b], dcnt[b])
    return idx, sc, cnt, status


@pytest.mark.parametrize("k_cls", [257, 1203, 4100])
def test_candidate_set_is_bit_identical_and_select_equals_the_dense_topk(k_cls):
    from wedetect_amd import sparse as SP
    c = _dense(k_cls)
    thr = _kth_largest(c["out_np"], 10000)
    n_ref = _counts(c, thr)
    print(f"K {k_cls}: thr {thr:.6g}, candidates per image {n_ref}")
    assert all(2000 <= n <= 8000 for n in n_ref)
    cap = 8192
    ref, seen_ref = R.lists(c["out_np"], B, thr)
    assert seen_ref.tolist() == n_ref
    # the independent producer: wd_sparse_rows over the dense output
    lr, sr, raw_r, sraw_r = _buffers(cap)
    SP.sparse_rows(c["out"], B, NTOT, k_cls, k_cls, k_cls, thr, lr, cap, sr)
    rows_keys, rows_seen = _sorted_lists(lr, sr, cap)
    # the fused kernel
    lf, sf, raw_f, sraw_f = _buffers(cap)
    flag = torch.zeros(1, dtype=torch.int32, device="cuda")
    _fused(c, thr, lf, cap, sf, flag=flag)
    fused_keys, fused_seen = _sorted_lists(lf, sf, cap)
    assert int(flag) == 0
    for b in range(B):
        assert _same(fused_keys[b], rows_keys[b]) and _same(fused_keys[b], ref[b])
    assert fused_seen.tolist() == n_ref and rows_seen.tolist() == n_ref
    assert not bool(sf[:, 1].any()) and not bool(sr[:, 1].any())
    for raw, n in ((raw_r, B * cap), (raw_f, B * cap)):
        assert bool((raw[n:] == POISON).all())
    for sraw in (sraw_r, sraw_f):
        assert bool((sraw[2 * B:] == POISON32).all())
    # select == dense top-k: no truncation, and truncation inside the list
    for nms_pre in (30000, 1000):
        list_cap = max(cap, 32768) if nms_pre == 30000 else cap  # the header: list_cap >= wd_topk_capacity(nms_pre) = 32768 for 30000
        l2, s2, _, _ = _buffers(list_cap)
        _fused(c, thr, l2, list_cap, s2)
        idx, sc, cnt, _ = _assert_select_equals_dense(c, thr, l2, list_cap, s2, nms_pre)
        assert cnt.tolist() == [min(n, nms_pre) for n in n_ref]
        for b in range(B):                                       # ... and the numpy restatement
            ridx, rsc, rn, _ = R.select(ref[b], n_ref[b], False, list_cap, nms_pre)
            assert np.array_equal(idx[b].cpu().numpy(), ridx) and _same(sc[b].cpu().numpy().view(np.uint32), rsc.view(np.uint32))
    # the bank as three chunks at multiples of eight rows, out of order: the same set, the same select output
    c1 = k_cls // 3 // 8 * 8
    lc, sc_, _, _ = _buffers(cap)
    _fused(c, thr, lc, cap, sc_, cuts=[(2 * c1, k_cls), (0, c1), (c1, 2 * c1)])
    chunk_keys, chunk_seen = _sorted_lists(lc, sc_, cap)
    assert chunk_seen.tolist() == n_ref and all(_same(chunk_keys[b], ref[b]) for b in range(B))
    first = _assert_select_equals_dense(c, thr, lc, cap, sc_, 1000)
    for _ in range(2):                                           # no race between runs
        l3, s3, _, _ = _buffers(cap)
        _fused(c, thr, l3, cap, s3)
        again = _select(l3, cap, s3, 1000)
        assert all(torch.equal(x, y) for x, y in zip(first, again))


def test_equal_scores_keep_the_dense_order_across_the_cut():
    """seg_scale (8, 8, 8): many pairs saturate to one score; the flat index breaks the ties, also where nms_pre cuts a run."""
    seg = (NTOT, ENDS[0], ENDS[1], (8.0, 8.0, 8.0), (-2.6, -2.2, -1.9))
    c = _dense(1203, seg)
    thr = _kth_largest(c["out_np"], 10000)
    n_ref = _counts(c, thr)
    assert all(1500 <= n <= 8000 for n in n_ref)
    s0 = np.sort(c["out_np"][:NTOT].reshape(-1))[::-1][:n_ref[0]]
    ties = int((np.diff(s0) == 0).sum())
    cut = [n for n in range(500, min(1500, n_ref[0])) if s0[n - 1] == s0[n]]
    print(f"thr {thr:.6g}, candidates {n_ref}, equal-score neighbours in image 0: {ties}, cuts inside a run: {len(cut)}")
    assert ties >= 10 and cut, "the case must hold equal scores inside the candidate set and a run across the cut"
    cap = 8192
    for nms_pre in (cut[len(cut) // 2], 8192):
        lst, state, _, _ = _buffers(cap)
        _fused(c, thr, lst, cap, state)
        _assert_select_equals_dense(c, thr, lst, cap, state, nms_pre)


def test_empty_and_overflowing_thresholds():
    c = _dense(257)
    lst, state, raw, _ = _buffers(1024)
    _fused(c, 1.0, lst, 1024, state)
    idx, sc, cnt, status = _select(lst, 1024, state, 1000)
    assert status.tolist() == [0, 0] and cnt.tolist() == [0, 0] and state[:, 0].tolist() == [0, 0]
    assert bool((idx == -1).all()) and not bool(sc.any()) and bool((raw == POISON).all())
    assert int((c["out"] > 0).sum()) == c["out"].numel()          # thr 0: every pair is a candidate
    lst, state, raw, _ = _buffers(1024)
    _fused(c, 0.0, lst, 1024, state)
    idx, sc, cnt, status = _select(lst, 1024, state, 1000)
    assert status.tolist() == [1, 1] and cnt.tolist() == [0, 0] and state[:, 0].tolist() == [NTOT * 257] * 2
    assert bool((idx == -1).all()) and not bool(sc.any()) and bool((raw[B * 1024:] == POISON).all())
    assert not bool((lst == POISON).any())                       # the lists are full


def test_overflow_of_one_image_leaves_the_other_exact():
    c = _dense(1203, img1_scale=0.25)
    thr = _kth_largest(c["out_np"][NTOT:], 500)
    n_ref = _counts(c, thr)
    print(f"thr {thr:.6g}, candidates per image {n_ref}")
    assert n_ref[0] > 1024 and 1 <= n_ref[1] <= 1024
    lst, state, _, _ = _buffers(1024)
    _fused(c, thr, lst, 1024, state)
    torch.cuda.synchronize()
    assert state[:, 0].tolist() == n_ref
    idx, sc, cnt, status = _select(lst, 1024, state, 1000)
    didx, dsc, dcnt = _dense_topk(c["out"], NTOT * 1203, thr, 1000)
    assert status.tolist() == [1, 0] and int(cnt[0]) == 0 and bool((idx[0] == -1).all())
    assert torch.equal(idx[1], didx[1]) and torch.equal(sc[1], dsc[1]) and int(cnt[1]) == int(dcnt[1]) == n_ref[1]


def test_non_finite_accumulator_raises_the_flag_and_marks_its_image_only():
    from wedetect_amd import lib as L
    from wedetect_amd import sparse as SP
    k_cls, rows = 257, B * NTOT
    e = _rand((rows, DIM), 311)
    e[5, 100] = 1e6                                              # hi half = inf
    t = torch.nn.functional.normalize(_rand((k_cls, DIM), 312), dim=-1)
    es, ts = _to_split_padded(e), L.split_weights(t)
    out = torch.empty(rows, k_cls, device="cuda")
    L.similarity_split(es, rows, ts[0], ts[1], out, k_cls, DIM, k_cls, seg=SEG, sigmoid=True)
    torch.cuda.synchronize()
    thr = _kth_largest(out[NTOT:].cpu().numpy(), 3000)
    flag = torch.zeros(1, dtype=torch.int32, device="cuda")
    lst, state, _, _ = _buffers(8192)
    SP.sparse_similarity_split(es, rows, ts[0], ts[1], k_cls, DIM, NTOT, k_cls, thr, lst, 8192, state, seg=SEG, range_flag=flag)
    idx, sc, cnt, status = _select(lst, 8192, state, 1000)
    assert int(flag) == 1 and state[:, 1].tolist() == [1, 0]
    didx, dsc, dcnt = _dense_topk(out, NTOT * k_cls, thr, 1000)
    assert status.tolist() == [2, 0] and int(cnt[0]) == -1 and int(dcnt[0]) == -1
    assert torch.equal(idx[1], didx[1]) and torch.equal(sc[1], dsc[1]) and int(cnt[1]) == int(dcnt[1]) == 1000
    # wd_sparse_rows sees the non-finite score of the materialised block
    lst, state, _, _ = _buffers(8192)
    SP.sparse_rows(out, B, NTOT, k_cls, k_cls, k_cls, thr, lst, 8192, state)
    torch.cuda.synchronize()
    assert state[:, 1].tolist() == [1, 0]


def test_sparse_rows_with_counts_and_a_class_offset_against_numpy():
    from wedetect_amd import sparse as SP
    n_img, rpi, k, ld, off, k_total, cap, thr = 3, 37, 80, 96, 1000, 1200, 4096, 0.5
    g = np.random.default_rng(3)
    sc = (np.round(g.random((n_img * rpi, ld), dtype=np.float32) * 32) / 32).astype(np.float32)
    sc[:, k:] = 2.0                                              # beyond n_cls: never read
    counts = np.asarray([1, 7, 80], np.int32)
    lst, state, raw, sraw = _buffers(cap, n_img)
    SP.sparse_rows(torch.from_numpy(sc).cuda(), n_img, rpi, k, ld, k_total, thr, lst, cap, state, cls_offset=off,
                   count=torch.from_numpy(counts).cuda())
    keys, seen = _sorted_lists(lst, state, cap)
    for b in range(n_img):
        want = R.image_list(sc[b * rpi:(b + 1) * rpi, :k], thr, n_cls_total=k_total, cls_offset=off, count=int(counts[b]))
        assert int(seen[b]) == want.shape[0] > 0 and _same(keys[b], want)
        s, flat = R.unpack_key(keys[b])
        assert bool((flat % k_total >= off).all()) and bool((flat % k_total < off + counts[b]).all()) and bool((s > thr).all())
    assert bool((raw[n_img * cap:] == POISON).all()) and bool((sraw[2 * n_img:] == POISON32).all()) and not bool(state[:, 1].any())
    # count NULL reads n_cls columns; a second producer appends behind the first
    lst, state, _, _ = _buffers(cap, n_img)
    d = torch.from_numpy(sc).cuda()
    SP.sparse_rows(d[:, :48].contiguous(), n_img, rpi, 48, 48, k_total, thr, lst, cap, state, cls_offset=off)
    SP.sparse_rows(d[:, 48:].contiguous(), n_img, rpi, k - 48, ld - 48, k_total, thr, lst, cap, state, cls_offset=off + 48)
    keys, seen = _sorted_lists(lst, state, cap)
    for b in range(n_img):
        assert _same(keys[b], R.image_list(sc[b * rpi:(b + 1) * rpi, :k], thr, n_cls_total=k_total, cls_offset=off))


def test_sparse_entries_refuse_bad_arguments_with_the_documented_codes():
    from wedetect_amd import lib as L
    from wedetect_amd import sparse as SP
    c = _dense(257)
    lst, state, raw, _ = _buffers(1024)
    sc = torch.zeros(8, 4, device="cuda")
    out = [torch.zeros(B * 1024, dtype=torch.int32, device="cuda") for _ in range(4)]
    cases = [
        (-1, lambda: SP.sparse_rows(sc, 2, 4, 4, 4, 4, 0.5, lst.data_ptr() + 4, 1024, state)),               # a misaligned list
        (-1, lambda: _fused(c, 0.5, lst.data_ptr() + 4, 1024, state)),
        (-1, lambda: SP.sparse_select(lst.data_ptr() + 4, 1024, state, B, 1000, *out)),
        (-1, lambda: SP.sparse_rows(sc, 2, 4, 4, 4, 4, 0.5, lst, 1000, state)),                              # not a power of two
        (-1, lambda: _fused(c, 0.5, lst, 1000, state)),
        (-1, lambda: SP.sparse_select(lst, 1000, state, B, 1000, *out)),
        (-1, lambda: SP.sparse_select(lst, 512, state, B, 1000, *out)),                                      # list_cap < the top-k capacity
        (-1, lambda: SP.sparse_rows(sc, 2, 4, 5, 4, 5, 0.5, lst, 1024, state)),                              # ld < n_cls
        (-4, lambda: SP.sparse_rows(sc, 2, 4, 4, 4, 1 << 29, 0.5, lst, 1024, state)),                        # 4 * 2^29 = 2^31
        (-4, lambda: _fused(c, 0.5, lst, 1024, state, k_total=(1 << 31) // NTOT + 1)),
    ]
    for code, fn in cases:
        with pytest.raises(L.WedetectHipError, match=rf"\({code}\)$"):
            fn()
    torch.cuda.synchronize()
    assert bool((raw == POISON).all()) and not bool(state.any())
