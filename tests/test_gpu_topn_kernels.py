"""The device entry points of include/wedetect_hip_topn.h (GPU): the fused similarity + per-row top-n against the materialising
launch it must equal bit for bit, against tests/topn_ref.py, against float64, its tie rule, the row affine, its range flag;
wd_topn_rows / wd_topn_unpack / wd_topn_kept against numpy.

Shapes: those of tests/test_gpu_best_kernels.py — 2 x 525 rows (no multiple of 256 or 8, a row tile straddles both images, waves
straddle the level boundaries at 400 and 500), banks of 257 / 1203 / 4100 rows (2, 5 and 17 column tiles of 256: a ragged last
tile, more than one group of eight).  Keys are allocated with three poisoned words behind them."""
import functools

import numpy as np
import pytest
import torch

import tests.best_hazards  # noqa: F401
import tests.topn_hazards  # noqa: F401
from tests import topn_ref as R
from tests.test_gpu_best_kernels import DIM, ENDS, ES_SCALE, NTOT, POISON, SEG, _operands
from tests.test_gpu_split import _rand, _to_split_padded

pytestmark = pytest.mark.gpu

SEG_SAT = (NTOT, ENDS[0], ENDS[1], (8.0, 8.0, 8.0), (-2.6, -2.2, -1.9))
NS = (1, 2, 5, 8)


def _keys(rows, n):
    key = torch.zeros(rows * n + 3, dtype=torch.int64, device="cuda")
    key[rows * n:] = POISON
    return key


def _np_keys(key, rows, n):
    return key[: rows * n].view(rows, n).cpu().numpy().view(np.uint64)


@functools.lru_cache(maxsize=4)
def _case(k_cls, sat=False, plant=True):
    """Operands, their splits and the materialised scores of wd_similarity_split — computed once, shared, never written again."""
    from wedetect_amd import lib as L
    b = 2
    rows = b * NTOT
    seg = SEG_SAT if sat else SEG
    e, t = _operands(b, k_cls, plant)
    es, ts = _to_split_padded(e, ES_SCALE), L.split_weights(t)
    flag = torch.zeros(1, dtype=torch.int32, device="cuda")
    out = torch.empty(rows, k_cls, device="cuda")
    L.similarity_split(es, rows, ts[0], ts[1] / ES_SCALE, out, k_cls, DIM, k_cls, seg=seg, sigmoid=True, range_flag=flag)
    torch.cuda.synchronize()
    assert int(flag) == 0
    return dict(b=b, rows=rows, e=e, t=t, es=es, ts=ts, out=out, out_np=out.cpu().numpy(), seg=seg, flag=flag)


def _fused(c, k_cls, n, cuts=((0, None),)):
    from wedetect_amd import topn as TN
    key = _keys(c["rows"], n)
    for a, z in cuts:
        z = k_cls if z is None else z
        TN.topn_similarity_split(c["es"], c["rows"], c["ts"][0], c["ts"][1] / ES_SCALE, z - a, DIM, n, key, a, seg=c["seg"],
                                 range_flag=c["flag"], t_row=a)
    torch.cuda.synchronize()
    assert int(c["flag"]) == 0 and bool((key[c["rows"] * n:] == POISON).all())        # the poison behind the keys is intact
    return key


@pytest.mark.parametrize("k_cls", [257, 1203, 4100])
def test_fused_kernel_equals_the_materialised_scores_bit_for_bit(k_cls):
    from wedetect_amd import best as BS
    from wedetect_amd import topn as TN
    c = _case(k_cls)
    rows, b = c["rows"], c["b"]
    kbest = torch.zeros(rows, dtype=torch.int64, device="cuda")
    BS.best_similarity_split(c["es"], rows, c["ts"][0], c["ts"][1] / ES_SCALE, k_cls, DIM, kbest, 0, seg=SEG)
    slot0 = None
    for n in NS:
        kf = _fused(c, k_cls, n)
        kr = _keys(rows, n)
        TN.topn_rows(c["out"], b, NTOT, k_cls, k_cls, n, kr)
        torch.cuda.synchronize()
        assert torch.equal(kf, kr), f"n {n}: fused keys differ from wd_topn_rows over the materialised scores"
        ws, wl = R.top_n(c["out_np"], n)
        assert np.array_equal(_np_keys(kf, rows, n), TN.pack(ws, wl)), f"n {n}: keys differ from topn_ref"
        if n == 1:
            assert torch.equal(kf[:rows], kbest)               # n = 1 IS the best-class key
            slot0 = kf[:rows].clone()
        assert torch.equal(kf[: rows * n].view(rows, n)[:, 0], slot0), f"n {n}: slot 0 differs from the n = 1 result"
        # the bank in three chunks (starts at multiples of eight rows), issued out of order: the same keys
        c1 = k_cls // 3 // 8 * 8
        assert torch.equal(_fused(c, k_cls, n, ((2 * c1, k_cls), (0, c1), (c1, 2 * c1))), kf), f"n {n}: chunked"
        for _ in range(2):                                     # no race between runs
            assert torch.equal(_fused(c, k_cls, n), kf), f"n {n}: run to run"
    # the planted identical bank rows: neighbours in class order
    _, lab = TN.unpack(_np_keys(_fused(c, k_cls, 2), rows, 2))
    assert lab[401].tolist() == [9, k_cls - 2] and lab[7, 0] == 0 and lab[NTOT + 3, 0] == k_cls - 1


@pytest.mark.parametrize("k_cls", [1203, 4100])
def test_ties_go_to_the_lowest_classes(k_cls):
    """seg_scale (8, 8, 8): the scores saturate, most rows hold equal fp32 scores inside their top nine; among equals the lowest
    classes come first — a ranking by logits would answer differently."""
    from wedetect_amd import topn as TN
    c = _case(k_cls, sat=True, plant=False)
    rows = c["rows"]
    top9 = -np.sort(-c["out_np"], axis=1)[:, :9]
    tied = int((np.diff(top9, axis=1) == 0).any(axis=1).sum())
    print(f"K {k_cls}: rows with equal scores inside their top nine {tied}/{rows}")
    assert tied >= 100, "the case must hold rows with ties"
    kf = _fused(c, k_cls, 8)
    ws, wl = R.top_n(c["out_np"], 8)
    assert np.array_equal(_np_keys(kf, rows, 8), TN.pack(ws, wl))
    logits = (c["e"].double() @ c["t"].double().T)
    by_logit = logits.topk(8, dim=1).indices.cpu().numpy()
    assert int((by_logit != wl).any(axis=1).sum()) >= 1


@pytest.mark.parametrize("k_cls", [257, 1203, 4100])
def test_fused_kernel_against_float64(k_cls):
    """Sorted scores within 2e-6 of the float64 top 8 (what wd_similarity_split is held to); labels equal to the float64 ranking
    on every row whose eight consecutive float64 gaps among its top nine all exceed 4e-6 (twice that bound) — at most 1 % of
    the rows may be left out."""
    from wedetect_amd import topn as TN
    c = _case(k_cls, plant=False)
    rows = c["rows"]
    s, lab = TN.unpack(_np_keys(_fused(c, k_cls, 8), rows, 8))
    lvl = torch.arange(rows, device="cuda") % NTOT
    lvl = (lvl >= ENDS[0]).long() + (lvl >= ENDS[1]).long()
    sc = torch.tensor(SEG[3], device="cuda", dtype=torch.float64)[lvl][:, None]
    bi = torch.tensor(SEG[4], device="cuda", dtype=torch.float64)[lvl][:, None]
    ref = torch.sigmoid((c["e"].double() @ c["t"].double().T) * sc + bi)
    top9 = ref.topk(9, dim=1)
    err = float((torch.from_numpy(s).cuda().double() - top9.values[:, :8]).abs().max())
    decided = ((top9.values[:, :8] - top9.values[:, 1:]) > 4e-6).all(dim=1)
    left_out = int((~decided).sum())
    print(f"K {k_cls}: max |top score - float64| {err:.3g}, rows left out {left_out}/{rows}")
    assert err <= 2e-6
    assert left_out <= rows // 100
    assert torch.equal(torch.from_numpy(lab).cuda().long()[decided], top9.indices[:, :8][decided])


def test_row_affine_fused_and_rows_forms_agree_and_match_float64():
    from wedetect_amd import lib as L
    from wedetect_amd import topn as TN
    k_cls, n = 1203, 8
    c = _case(k_cls)
    rows, b = c["rows"], c["b"]
    g = torch.Generator().manual_seed(41)
    rs = (torch.rand(rows, generator=g) * 1.5 + 0.2).cuda()
    rb = (torch.rand(rows, generator=g) * 2 - 3).cuda()
    logits = torch.empty(rows, k_cls, device="cuda")
    unit = (NTOT, ENDS[0], ENDS[1], (1.0, 1.0, 1.0), (0.0, 0.0, 0.0))      # scale 1, bias 0, no sigmoid: the raw logits
    L.similarity_split(c["es"], rows, c["ts"][0], c["ts"][1] / ES_SCALE, logits, k_cls, DIM, k_cls, seg=unit, sigmoid=False)
    kf, kr = _keys(rows, n), _keys(rows, n)
    TN.topn_similarity_split(c["es"], rows, c["ts"][0], c["ts"][1] / ES_SCALE, k_cls, DIM, n, kf, 0, row_scale=rs, row_bias=rb, range_flag=c["flag"])
    TN.topn_rows(logits, b, NTOT, k_cls, k_cls, n, kr, row_scale=rs, row_bias=rb)
    torch.cuda.synchronize()
    assert int(c["flag"]) == 0 and torch.equal(kf, kr)
    s, lab = TN.unpack(_np_keys(kf, rows, n))
    ref = torch.sigmoid((c["e"].double() @ c["t"].double().T) * rs.double().exp()[:, None] + rb.double()[:, None])
    top = ref.topk(n, dim=1).values
    err = float((torch.from_numpy(s).cuda().double() - top).abs().max())
    err_lab = float((torch.gather(ref, 1, torch.from_numpy(lab).cuda().long()) - top).abs().max())
    print(f"row affine: max |score - float64| {err:.3g}, through the labels {err_lab:.3g}")
    assert err <= 2e-6 and err_lab <= 4e-6
    with pytest.raises(L.WedetectHipError):                   # both affines
        TN.topn_similarity_split(c["es"], rows, c["ts"][0], c["ts"][1] / ES_SCALE, k_cls, DIM, n, kf, 0, seg=SEG, row_scale=rs, row_bias=rb)
    with pytest.raises(L.WedetectHipError):                   # half a row affine
        TN.topn_similarity_split(c["es"], rows, c["ts"][0], c["ts"][1] / ES_SCALE, k_cls, DIM, n, kf, 0, row_scale=rs)
    for bad_n in (0, 9):
        with pytest.raises(L.WedetectHipError):
            TN.topn_similarity_split(c["es"], rows, c["ts"][0], c["ts"][1] / ES_SCALE, k_cls, DIM, bad_n, kf, 0, seg=SEG)
    torch.cuda.synchronize()
    assert torch.equal(kf, kr)                                # a refused call touched nothing


def test_topn_rows_edge_cases_against_numpy():
    from wedetect_amd import topn as TN
    g = np.random.default_rng(3)
    d = lambda a: torch.from_numpy(a).cuda()
    # K = 3 with n = 5: slots 3 and 4 stay empty
    sc = g.random((10, 3), dtype=np.float32)
    key = _keys(10, 5)
    TN.topn_rows(d(sc), 2, 5, 3, 3, 5, key)
    torch.cuda.synchronize()
    ws, wl = R.top_n(sc, 5)
    assert np.array_equal(_np_keys(key, 10, 5), TN.pack(ws, wl)) and bool((wl[:, 3:] == -1).all()) and bool((key[50:] == POISON).all())
    # ragged counts (0, a few, above n_cls), ld > n_cls with NaN in the spare columns, ties in most rows, two blocks with offsets
    n_img, rpi, k, ld, n = 4, 37, 70, 83, 8
    full = (np.round(g.random((n_img * rpi, 2 * k), dtype=np.float32) * 32) / 32).astype(np.float32)
    counts = np.asarray([0, 3, 2 * k + 9, 75], np.int32)      # image 3: all of block 0, five columns of block 1
    key = _keys(n_img * rpi, n)
    for blk in (1, 0):                                        # out of order
        part = np.full((n_img * rpi, ld), np.nan, np.float32)
        part[:, :k] = full[:, blk * k:(blk + 1) * k]
        cnt = np.clip(counts - blk * k, 0, None).astype(np.int32)
        TN.topn_rows(d(part), n_img, rpi, k, ld, n, key, 1000 + blk * k, d(cnt))
    torch.cuda.synchronize()
    want = np.zeros((n_img * rpi, n), np.uint64)
    for r in range(n_img * rpi):
        m = min(int(counts[r // rpi]), 2 * k)
        if m:
            ws, wl = R.top_n(full[r:r + 1, :m], n)
            want[r] = TN.pack(ws, np.where(wl >= 0, wl + 1000, -1))[0]
    assert np.array_equal(_np_keys(key, n_img * rpi, n), want) and bool((key[n_img * rpi * n:] == POISON).all())
    assert not want[:rpi].any() and int((want[rpi:2 * rpi] != 0).sum(axis=1).max()) == 3
    # count NULL reads n_cls columns of every row
    key = _keys(n_img * rpi, n)
    TN.topn_rows(d(full), n_img, rpi, k, 2 * k, n, key)
    torch.cuda.synchronize()
    ws, wl = R.top_n(full[:, :k], n)
    assert np.array_equal(_np_keys(key, n_img * rpi, n), TN.pack(ws, wl))


def test_unpack_and_kept_against_numpy():
    from wedetect_amd import lib as L
    from wedetect_amd import topn as TN
    g = np.random.default_rng(8)
    b, n_anchor, n, max_out = 3, 50, 5, 7
    rows = b * n_anchor
    ks, kl = R.top_n(g.random((rows, 4), dtype=np.float32), n)      # slot 4 of every row is empty
    key = torch.from_numpy(TN.pack(ks, kl).view(np.int64)).cuda()
    for slot in (0, 3, 4):
        s = torch.full((rows + 2,), 7.0, device="cuda")
        lab = torch.full((rows + 2,), 77, dtype=torch.int32, device="cuda")
        TN.topn_unpack(key, rows, n, slot, s, lab)
        torch.cuda.synchronize()
        assert bool((s[rows:] == 7.0).all()) and bool((lab[rows:] == 77).all())
        assert np.array_equal(s[:rows].cpu().numpy(), ks[:, slot]) and np.array_equal(lab[:rows].cpu().numpy(), kl[:, slot])
    assert bool((kl[:, 4] == -1).all())
    counts = np.asarray([0, max_out, 4], np.int32)
    anc = g.integers(0, n_anchor, (b, max_out)).astype(np.int32)
    anc[2, 1], anc[2, 2] = n_anchor, -1                      # out of range
    ts = torch.full((b * max_out * n + 2,), 7.0, device="cuda")
    tl = torch.full((b * max_out * n + 2,), 77, dtype=torch.int32, device="cuda")
    TN.topn_kept(key, n, n_anchor, torch.from_numpy(anc).cuda(), torch.from_numpy(counts).cuda(), max_out, b, ts, tl)
    torch.cuda.synchronize()
    assert bool((ts[-2:] == 7.0).all()) and bool((tl[-2:] == 77).all())
    s, lab = ts[:-2].view(b, max_out, n).cpu().numpy(), tl[:-2].view(b, max_out, n).cpu().numpy()
    for i in range(b):
        for r in range(max_out):
            a = int(anc[i, r])
            if r < counts[i] and 0 <= a < n_anchor:
                assert np.array_equal(s[i, r], ks[i * n_anchor + a]) and np.array_equal(lab[i, r], kl[i * n_anchor + a])
            else:
                assert not s[i, r].any() and bool((lab[i, r] == -1).all())
    with pytest.raises(L.WedetectHipError):
        TN.topn_unpack(key, rows, n, n, ts, tl)              # slot outside [0, n_top)
    with pytest.raises(L.WedetectHipError):
        TN.topn_rows(ts, 2, 4, 5, 4, 3, key)                 # ld < n_cls
    with pytest.raises(L.WedetectHipError):
        TN.topn_rows(ts, 2, 4, 4, 4, 3, key.data_ptr() + 4)  # a misaligned key


def test_fused_kernel_raises_its_range_flag_and_gives_the_row_a_non_finite_score():
    from wedetect_amd import lib as L
    from wedetect_amd import topn as TN
    rows, k_cls, n = 64, 16, 5
    e = _rand((rows, DIM), 311)
    good = e.clone()
    e[5, 100] = 1e6                                           # hi half = inf
    t = torch.nn.functional.normalize(_rand((k_cls, DIM), 312), dim=-1)
    ts = L.split_weights(t)
    seg = (rows, 32, 48, (1.0, 1.0, 1.0), (0.0, 0.0, 0.0))
    keys = []
    for src, want_flag in ((e, 1), (good, 0)):
        flag = torch.zeros(1, dtype=torch.int32, device="cuda")
        key = torch.zeros(rows, n, dtype=torch.int64, device="cuda")
        TN.topn_similarity_split(_to_split_padded(src), rows, ts[0], ts[1], k_cls, DIM, n, key, 0, seg=seg, range_flag=flag)
        torch.cuda.synchronize()
        assert int(flag) == want_flag
        keys.append(key.cpu().numpy().view(np.uint64))
    s, _ = TN.unpack(keys[0])
    other = np.arange(rows) != 5
    assert not np.isfinite(s[5, 0]) and bool(np.isfinite(s[other]).all())
    assert np.array_equal(keys[0][other], keys[1][other])      # the other rows: the lists of the clean run ...
    out = torch.empty(rows, k_cls, device="cuda")
    L.similarity_split(_to_split_padded(good), rows, ts[0], ts[1], out, k_cls, DIM, k_cls, seg=seg, sigmoid=True)
    ws, wl = R.top_n(out.cpu().numpy(), n)
    assert np.array_equal(keys[1], TN.pack(ws, wl))            # ... which are the reference's
