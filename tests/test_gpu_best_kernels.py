"""The device entry points of include/wedetect_hip_best.h (GPU): the fused similarity + class argmax against the materialising
launch it must equal bit for bit, against float64, its range flag; wd_best_rows / wd_best_unpack against numpy;
wd_nms_gather_labeled against tests/best_ref.py and against wd_nms_gather.

Shapes: 2 x 525 rows (no multiple of 256 or 8, a row tile straddles both images, waves straddle the level boundaries at 400
and 500), banks of 257 / 1203 / 4100 rows (2, 5 and 17 column tiles of 256: a ragged last tile, more than one group of eight)."""
import numpy as np
import pytest
import torch

import tests.best_hazards  # noqa: F401
from tests import best_ref as R
from tests.test_gpu_split import _rand, _to_split_padded

pytestmark = pytest.mark.gpu

NTOT, ENDS, DIM, ES_SCALE = 525, (400, 500), 768, 4.0
SEG = (NTOT, ENDS[0], ENDS[1], (1.9, 1.6, 2.2), (-2.6, -2.2, -1.9))
POISON = 0x5555555555555555


def _operands(b, k_cls, plant):
    rows = b * NTOT
    e = _rand((rows, DIM), 301, 0.8)
    t = torch.nn.functional.normalize(_rand((k_cls, DIM), 302), dim=-1)
    if plant:
        unit = lambda r: torch.nn.functional.normalize(e[r], dim=-1)
        t[0] = unit(7)                                       # row 7: the best class is class 0
        t[k_cls - 1] = unit(NTOT + 3)                        # row 528: ... the last class of the ragged tile
        t[9] = unit(401)                                     # row 401: two identical bank rows, the lower index wins
        t[k_cls - 2] = t[9]
    return e, t


def _keys(rows):
    key = torch.zeros(rows + 3, dtype=torch.int64, device="cuda")
    key[rows:] = POISON
    return key


def _unpack(key, rows):
    from wedetect_amd import best as BS
    s = torch.full((rows + 2,), 7.0, device="cuda")
    lab = torch.full((rows + 2,), 77, dtype=torch.int32, device="cuda")
    BS.best_unpack(key, rows, s, lab)
    torch.cuda.synchronize()
    assert bool((s[rows:] == 7.0).all()) and bool((lab[rows:] == 77).all())
    return s[:rows], lab[:rows]


def _fused_and_reference(b, k_cls, seg, plant=True):
    """(keys of the fused kernel, keys of wd_best_rows over wd_similarity_split's output, that output) on the same operands."""
    from wedetect_amd import best as BS
    from wedetect_amd import lib as L
    rows = b * NTOT
    e, t = _operands(b, k_cls, plant)
    es, ts = _to_split_padded(e, ES_SCALE), L.split_weights(t)
    flag = torch.zeros(1, dtype=torch.int32, device="cuda")
    out = torch.empty(rows, k_cls, device="cuda")
    L.similarity_split(es, rows, ts[0], ts[1] / ES_SCALE, out, k_cls, DIM, k_cls, seg=seg, sigmoid=True, range_flag=flag)
    kref, kfused = _keys(rows), _keys(rows)
    BS.best_rows(out, b, NTOT, k_cls, k_cls, kref)
    BS.best_similarity_split(es, rows, ts[0], ts[1] / ES_SCALE, k_cls, DIM, kfused, 0, seg=seg, range_flag=flag)
    torch.cuda.synchronize()
    assert int(flag) == 0
    return dict(e=e, t=t, es=es, ts=ts, out=out, kref=kref, kfused=kfused, rows=rows)


@pytest.mark.parametrize("k_cls", [257, 1203, 4100])
def test_fused_kernel_equals_the_materialised_scores_bit_for_bit(k_cls):
    from wedetect_amd import best as BS
    c = _fused_and_reference(2, k_cls, SEG)
    rows, out = c["rows"], c["out"]
    assert torch.equal(c["kfused"], c["kref"])
    assert bool((c["kfused"][rows:] == POISON).all())        # rows past the count keep their poison
    s, lab = _unpack(c["kfused"], rows)
    s_ref, lab_ref = _unpack(c["kref"], rows)
    assert torch.equal(s, s_ref) and torch.equal(lab, lab_ref)
    best, arg = R.best_class(out.cpu().numpy())              # numpy max / argmax (first occurrence) of the materialised block
    assert np.array_equal(s.cpu().numpy().view(np.uint32), best.view(np.uint32)) and np.array_equal(lab.cpu().numpy(), arg)
    # the planted rows
    assert int(lab[7]) == 0 and int(lab[NTOT + 3]) == k_cls - 1 and int(lab[401]) == 9
    assert float(out[401, 9]) == float(out[401, k_cls - 2]) == float(s[401])
    # the bank in three chunks (starts at multiples of eight rows), issued out of order: the same keys
    c1 = k_cls // 3 // 8 * 8
    cuts = [(2 * c1, k_cls), (0, c1), (c1, 2 * c1)]
    kc = _keys(rows)
    for a, z in cuts:
        BS.best_similarity_split(c["es"], rows, c["ts"][0], c["ts"][1] / ES_SCALE, z - a, DIM, kc, a, seg=SEG, t_row=a)
    torch.cuda.synchronize()
    assert torch.equal(kc, c["kfused"])
    for _ in range(2):                                       # no race between runs
        k2 = _keys(rows)
        BS.best_similarity_split(c["es"], rows, c["ts"][0], c["ts"][1] / ES_SCALE, k_cls, DIM, k2, 0, seg=SEG)
        torch.cuda.synchronize()
        assert torch.equal(k2, c["kfused"])


def test_fused_kernel_keeps_the_lowest_class_among_saturated_scores():
    """seg_scale (8, 8, 8): several classes of a row saturate to the same score; the sigmoid is applied per element, so the
    label is the lowest of them — not the class of the largest logit."""
    seg = (NTOT, ENDS[0], ENDS[1], (8.0, 8.0, 8.0), (-2.6, -2.2, -1.9))
    c = _fused_and_reference(2, 1203, seg, plant=False)
    out = c["out"]
    ties = (out == out.max(dim=1, keepdim=True).values).sum(dim=1)
    assert int((ties > 1).sum()) >= 10, "the case must hold rows with several classes at the maximum"
    assert torch.equal(c["kfused"], c["kref"])
    s, lab = _unpack(c["kfused"], c["rows"])
    best, arg = R.best_class(out.cpu().numpy())
    assert np.array_equal(s.cpu().numpy(), best) and np.array_equal(lab.cpu().numpy(), arg)
    logits = (c["e"].double() @ c["t"].double().T)
    assert int((logits.argmax(dim=1).cpu() != lab.cpu()).sum()) >= 1     # a maximum of logits would have answered differently


@pytest.mark.parametrize("b,k_cls", [(2, 257), (2, 1203), (2, 4100), (1, 20000)])
def test_fused_kernel_against_float64(b, k_cls):
    """best_score within 2e-6 of the float64 maximum (what wd_similarity_split is held to); best_label equal to the float64
    argmax on every row whose float64 top-two gap exceeds 4e-6 (twice that bound: a smaller gap is inside the scores' own
    error) — at most 1 % of the rows may be left out."""
    from wedetect_amd import best as BS
    from wedetect_amd import lib as L
    rows = b * NTOT
    e, t = _operands(b, k_cls, plant=False)
    es, ts = _to_split_padded(e, ES_SCALE), L.split_weights(t)
    key = _keys(rows)
    BS.best_similarity_split(es, rows, ts[0], ts[1] / ES_SCALE, k_cls, DIM, key, 0, seg=SEG)
    s, lab = _unpack(key, rows)
    lvl = torch.arange(rows, device="cuda") % NTOT
    lvl = (lvl >= ENDS[0]).long() + (lvl >= ENDS[1]).long()
    sc = torch.tensor(SEG[3], device="cuda", dtype=torch.float64)[lvl][:, None]
    bi = torch.tensor(SEG[4], device="cuda", dtype=torch.float64)[lvl][:, None]
    ref = torch.sigmoid((e.double() @ t.double().T) * sc + bi)
    top2 = ref.topk(2, dim=1)
    err = float((s.double() - top2.values[:, 0]).abs().max())
    gap = top2.values[:, 0] - top2.values[:, 1]
    decided = gap > 4e-6
    left_out = int((~decided).sum())
    print(f"K {k_cls}: max |best_score - float64| {err:.3g}, smallest top-two gap {float(gap.min()):.3g}, rows left out {left_out}/{rows}")
    assert err <= 2e-6
    assert left_out <= rows // 100
    assert torch.equal(lab.long()[decided], top2.indices[:, 0][decided])


def test_fused_kernel_raises_its_range_flag_and_gives_the_row_a_non_finite_score():
    from wedetect_amd import best as BS
    from wedetect_amd import lib as L
    rows, k_cls = 64, 16
    e = _rand((rows, DIM), 311)
    e[5, 100] = 1e6                                           # hi half = inf
    t = torch.nn.functional.normalize(_rand((k_cls, DIM), 312), dim=-1)
    ts = L.split_weights(t)
    flag = torch.zeros(1, dtype=torch.int32, device="cuda")
    seg = (rows, 32, 48, (1.0, 1.0, 1.0), (0.0, 0.0, 0.0))
    key = torch.zeros(rows, dtype=torch.int64, device="cuda")
    BS.best_similarity_split(_to_split_padded(e), rows, ts[0], ts[1], k_cls, DIM, key, 0, seg=seg, range_flag=flag)
    s, lab = _unpack(key, rows)
    assert int(flag) == 1
    finite = torch.isfinite(s)
    assert not bool(finite[5]) and bool(finite[torch.arange(rows, device="cuda") != 5].all())
    # ... which the top-k guard reports for the image
    idx = torch.empty(1, L.topk_capacity(100), dtype=torch.int32, device="cuda")
    sc, cnt = torch.empty(1, idx.shape[1], device="cuda"), torch.empty(1, dtype=torch.int32, device="cuda")
    ws = torch.empty(L.topk_workspace_bytes(1, rows, 100) + 256, dtype=torch.uint8, device="cuda")
    ws = ws[(-ws.data_ptr()) % 256:]
    L.topk_candidates(s, 1, rows, 0.0, 100, idx, sc, cnt, ws)
    assert int(cnt) == -1
    with pytest.raises(L.WedetectHipError):                   # dim % 32
        BS.best_similarity_split(_to_split_padded(e[:, :48].contiguous()), rows, ts[0], ts[1], k_cls, 48, key, 0, seg=seg)
    with pytest.raises(L.WedetectHipError):                   # a negative class offset
        BS.best_similarity_split(_to_split_padded(e), rows, ts[0], ts[1], k_cls, DIM, key, -1, seg=seg)


def test_best_rows_and_unpack_against_numpy():
    """Per-image counts 0 / 1 / k_max, ld > n_cls, a class offset, keys that already hold a better or a worse class."""
    from wedetect_amd import best as BS
    n_img, rpi, k, ld, off = 3, 37, 70, 83, 1000
    g = np.random.default_rng(3)
    sc = (np.round(g.random((n_img * rpi, ld), dtype=np.float32) * 32) / 32).astype(np.float32)       # ties in most rows
    sc[:, k:] = 2.0                                          # beyond n_cls: never read
    counts = np.asarray([0, 1, k], np.int32)
    key0 = np.zeros(n_img * rpi + 2, np.uint64)
    key0[2 * rpi] = BS.pack_key(np.float32(5.0).view(np.uint32), 3)                  # a better class from an earlier chunk stays
    key0[2 * rpi + 1] = BS.pack_key(np.float32(0.0).view(np.uint32), 3)              # a worse one is replaced
    key0[-2:] = POISON
    want = key0.copy()
    for r in range(n_img * rpi):
        n = int(counts[r // rpi])
        if n:
            want[r] = max(want[r], BS.pack_key(sc[r, :n].view(np.uint32), np.arange(n) + off).max())
    key = torch.from_numpy(key0.view(np.int64)).cuda()
    BS.best_rows(torch.from_numpy(sc).cuda(), n_img, rpi, k, ld, key, off, torch.from_numpy(counts).cuda())
    torch.cuda.synchronize()
    assert np.array_equal(key.cpu().numpy().view(np.uint64), want)
    s, lab = _unpack(key, n_img * rpi)
    ws, wl = BS.unpack_key(want[:-2])
    assert np.array_equal(s.cpu().numpy().view(np.uint32), ws.view(np.uint32)) and np.array_equal(lab.cpu().numpy(), wl)
    assert bool((lab[:rpi] == -1).all()) and bool((s[:rpi] == 0).all())               # count 0: no class seen
    assert bool((lab[rpi:2 * rpi] == off).all())                                        # count 1: class 0 of the chunk
    best, arg = R.best_class(sc[2 * rpi + 2:, :k])
    assert np.array_equal(s.cpu().numpy()[2 * rpi + 2:], best) and np.array_equal(lab.cpu().numpy()[2 * rpi + 2:], arg + off)
    # count NULL: every row reads n_cls columns
    key = torch.zeros(n_img * rpi, dtype=torch.int64, device="cuda")
    BS.best_rows(torch.from_numpy(sc).cuda(), n_img, rpi, k, ld, key)
    s, lab = _unpack(key, n_img * rpi)
    best, arg = R.best_class(sc[:, :k])
    assert np.array_equal(s.cpu().numpy(), best) and np.array_equal(lab.cpu().numpy(), arg)


def _nms_inputs(n_anchor=200, k=5, counts=(40, 150), dim=16, seed=21):
    g = np.random.default_rng(seed)
    b = len(counts)
    ctr = g.random((b, n_anchor, 2), dtype=np.float32) * 40 + 40          # dense: most candidates overlap a kept box
    wh = g.random((b, n_anchor, 2), dtype=np.float32) * 20 + 40
    boxes = np.concatenate([ctr - wh / 2, ctr + wh / 2], 2).astype(np.float32)
    labels = g.integers(0, k, (b, n_anchor)).astype(np.int32)
    cap = 256
    cidx, csc = np.full((b, cap), -1, np.int32), np.zeros((b, cap), np.float32)
    for i, n in enumerate(counts):
        cidx[i, :n] = g.permutation(n_anchor)[:n]
        csc[i, :n] = np.sort((np.round(g.random(n, dtype=np.float32) * 64) / 64 + np.float32(1 / 128)).astype(np.float32))[::-1]
    emb = g.standard_normal((b, n_anchor, dim)).astype(np.float32)
    return boxes, labels, cidx, csc, np.asarray(counts, np.int32), emb


@pytest.mark.parametrize("pre", [1.0, 0.0])
@pytest.mark.parametrize("agnostic", [False, True])
def test_nms_gather_labeled_is_bit_exact_against_the_reference(agnostic, pre):
    """WD_NMS_MMCV and WD_NMS_MMCV_AGNOSTIC, candidate counts on both sides of split_thr = 64 (40: one pass across labels;
    150: per label), both rescale orders, embeddings gathered; max_out 30 truncates the second image."""
    from wedetect_amd import best as BS
    from wedetect_amd import lib as L
    k, max_out, split_thr, dim = 5, 30, 64, 16
    boxes, labels, cidx, csc, counts, emb = _nms_inputs(k=k, dim=dim)
    b, n_anchor = labels.shape
    meta = np.asarray([[3.0, 5.0, 0.0, 0.5, 0.75, 300.0, 200.0, pre]] * b, np.float32)
    d = lambda a: torch.from_numpy(a).cuda()
    ob, os_ = torch.full((b, max_out, 4), 7.0, device="cuda"), torch.full((b, max_out), 7.0, device="cuda")
    ol, oa = (torch.full((b, max_out), 7, dtype=torch.int32, device="cuda") for _ in range(2))
    oc, oe = torch.full((b,), 7, dtype=torch.int32, device="cuda"), torch.full((b, max_out, dim), 7.0, device="cuda")
    ws = torch.full((max(1, L.nms_workspace_bytes(b) // 4),), -1, dtype=torch.int32, device="cuda")
    mode = BS.NMS_MMCV_AGNOSTIC if agnostic else L.NMS_MMCV
    BS.nms_gather_labeled(d(cidx), d(csc), d(counts), cidx.shape[1], d(boxes), n_anchor, d(labels), k, d(meta), L.nms_threshold(0.5, L.NMS_MMCV),
                          max_out, d(emb), dim, ob, os_, ol, oa, oc, oe, b, nms_mode=mode, mode_param=split_thr, workspace=ws)
    torch.cuda.synchronize()
    kept = []
    for i in range(b):
        n = int(counts[i])
        anc = cidx[i, :n].astype(np.int64)
        r = R.nms_rows(boxes[i][anc], csc[i, :n], labels[i][anc].astype(np.int64), meta[i], 0.5, max_out, split_thr, agnostic)
        keep = r["keep"]
        m = keep.shape[0]
        kept.append(m)
        assert int(oc[i]) == m
        assert np.array_equal(oa[i, :m].cpu().numpy(), anc[keep]) and np.array_equal(ol[i, :m].cpu().numpy(), labels[i][anc][keep])
        assert np.array_equal(os_[i, :m].cpu().numpy(), csc[i, :n][keep])
        assert np.array_equal(ob[i, :m].cpu().numpy().view(np.uint32), r["bboxes"].view(np.uint32))
        assert np.array_equal(oe[i, :m].cpu().numpy(), emb[i][anc[keep]])
        assert bool((oa[i, m:] == -1).all()) and bool((ol[i, m:] == -1).all()) and not bool(ob[i, m:].any()) and not bool(oe[i, m:].any())
    assert kept[1] == max_out and 0 < kept[0] < max_out
    if agnostic:                                             # the un-offset pass across labels keeps fewer rows than the offset one
        aware = R.nms_rows(boxes[0][cidx[0, :40]], csc[0, :40], labels[0][cidx[0, :40]].astype(np.int64), meta[0], 0.5, max_out, split_thr, False)
        assert aware["keep"].shape[0] > kept[0]


@pytest.mark.parametrize("nms,param", [("vanilla", 0), ("torchvision", 4000), ("torchvision", 100), ("mmcv", 10000), ("mmcv", 64)])
def test_nms_gather_labeled_reproduces_nms_gather(nms, param):
    """anchor_labels[b, a] = a % k and one candidate per anchor: the labeled form is wd_nms_gather on flat indices a * k + a % k."""
    from wedetect_amd import lib as L
    from wedetect_amd import best as BS
    k, max_out, dim = 5, 300, 16
    boxes, _, cidx, csc, counts, emb = _nms_inputs(k=k, dim=dim, seed=22)
    b, n_anchor = boxes.shape[:2]
    labels = np.broadcast_to(np.arange(n_anchor, dtype=np.int32) % k, (b, n_anchor)).copy()
    flat = np.where(cidx >= 0, cidx * k + cidx % k, -1).astype(np.int32)
    meta = np.asarray([[3.0, 5.0, 0.0, 0.5, 0.75, 300.0, 200.0, 1.0]] * b, np.float32)
    mode = {"vanilla": L.NMS_VANILLA, "torchvision": L.NMS_TORCHVISION, "mmcv": L.NMS_MMCV}[nms]
    d = lambda a: torch.from_numpy(a).cuda()
    outs = []
    for labeled in (False, True):
        o = [torch.full((b, max_out, 4), 7.0, device="cuda"), torch.full((b, max_out), 7.0, device="cuda"),
             torch.full((b, max_out), 7, dtype=torch.int32, device="cuda"), torch.full((b, max_out), 7, dtype=torch.int32, device="cuda"),
             torch.full((b,), 7, dtype=torch.int32, device="cuda"), torch.full((b, max_out, dim), 7.0, device="cuda")]
        ws = torch.zeros(max(1, L.nms_workspace_bytes(b) // 4), dtype=torch.int32, device="cuda")
        thr = L.nms_threshold(0.5, mode)
        if labeled:
            BS.nms_gather_labeled(d(cidx), d(csc), d(counts), cidx.shape[1], d(boxes), n_anchor, d(labels), k, d(meta), thr, max_out, d(emb),
                                  dim, o[0], o[1], o[2], o[3], o[4], o[5], b, nms_mode=mode, mode_param=param, workspace=ws)
        else:
            L.nms_gather(d(flat), d(csc), d(counts), cidx.shape[1], d(boxes), n_anchor, k, d(meta), thr, max_out, d(emb), dim,
                         o[0], o[1], o[2], o[3], o[4], o[5], b, nms_mode=mode, mode_param=param, workspace=ws)
        torch.cuda.synchronize()
        outs.append(o)
    for x, y in zip(*outs):
        assert torch.equal(x, y)
    assert int(outs[0][4].min()) > 0


def test_best_entries_refuse_bad_arguments():
    from wedetect_amd import best as BS
    from wedetect_amd import lib as L
    key = torch.zeros(8, dtype=torch.int64, device="cuda")
    sc = torch.zeros(8, 4, device="cuda")
    with pytest.raises(L.WedetectHipError):
        BS.best_rows(sc, 2, 4, 5, 4, key)                    # ld < n_cls
    with pytest.raises(L.WedetectHipError):
        BS.best_rows(sc, 2, 4, 4, 4, key.data_ptr() + 4)     # a misaligned key
    with pytest.raises(L.WedetectHipError):
        BS.best_unpack(key, 0, sc, sc)
    assert not bool(key.any())
