"""The exemplar kernels on the GPU (include/wedetect_hip_exemplar.h): wd_exemplar_assign against tests/exemplar_ref.py — anchors
AND IoU bits equal — at the smallest shapes where the selection can go wrong, wd_exemplar_pool against a float64 evaluation of the
definition within (S_c + 8) * 2^-23 and bit-identical across runs, class positions and class counts."""
import functools

import numpy as np
import pytest
import torch

import tests.exemplar_hazards  # noqa: F401
from tests import exemplar_ref as R

pytestmark = pytest.mark.gpu

f32 = np.float32
DIM = 768


@functools.lru_cache(maxsize=None)
def _boxes(n: int, batch: int):
    """Decoded-box look-alikes [batch, n, 4] on a 640-pixel canvas with few distinct sizes (IoU ties), duplicates of anchor 0's
    neighbourhood at distant anchors (other lanes, other waves, the last anchor) and a NaN box."""
    g = np.random.default_rng(1000 + n)
    xy = np.round(g.random((batch, n, 2), dtype=f32) * 560)
    wh = np.round(g.random((batch, n, 2), dtype=f32) * 3 + 1) * 16
    boxes = np.concatenate([xy, xy + wh], axis=2).astype(f32)
    for src, dst in ((0, 1), (0, 63), (0, 64), (0, 200), (0, 256), (0, 300), (0, 1023), (0, 1024), (0, n - 1), (5, 261), (5, 5 + 4 * 256)):
        if src < n and 0 < dst < n:
            boxes[:, dst] = boxes[:, src]
    if n > 40:
        boxes[:, 37, 0] = np.nan
    return boxes


@functools.lru_cache(maxsize=None)
def _case(n: int, batch: int, max_ex: int):
    """(boxes, ex_boxes in original pixels, ex_count, meta): example e of an image is the box of anchor (7 e) % n pushed by a few
    pixels (e even: not at all, so the duplicates tie at IoU 1), one example far from every box, ragged counts with a 0."""
    boxes = _boxes(n, batch)
    g = np.random.default_rng(7 * n + max_ex)
    meta = np.zeros((batch, 8), f32)
    meta[:, 0], meta[:, 1] = [3.0, 0.0, 11.5][:batch], [0.0, 7.25, 2.0][:batch]
    meta[:, 3], meta[:, 4] = [0.5, 1.0, f32(1 / 3)][:batch], [0.5, 1.0, f32(0.4)][:batch]
    meta[:, 5:7] = 2000
    ex = np.zeros((batch, max_ex, 4), f32)
    for b in range(batch):
        for e in range(max_ex):
            net = boxes[b, (7 * e) % n].copy()
            if np.isnan(net).any():
                net = boxes[b, 0].copy()
            if e % 2:
                net += np.round(g.random(4, dtype=f32) * 8 - 4)
            if e == 3:
                net = np.array([5000, 5000, 5040, 5040], f32)                 # matches nothing
            ex[b, e] = (net - np.array([meta[b, 0], meta[b, 1]] * 2, f32)) / np.array([meta[b, 3], meta[b, 4]] * 2, f32)
    cnt = np.array([max_ex, 0, max(1, max_ex - 3)][:batch], np.int32)
    if batch == 1:
        cnt[0] = max_ex
    return boxes, ex, cnt, meta


def _run_assign(boxes, ex, cnt, meta, m, thr):
    from wedetect_amd import exemplar as EX
    batch, n, _ = boxes.shape
    max_ex = ex.shape[1]
    d = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    sa = torch.full((batch, max_ex * m), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
    si = torch.full((batch, max_ex * m), float("nan"), dtype=torch.float32, device="cuda")
    sc = torch.full((batch,), -7, dtype=torch.int32, device="cuda")
    EX.exemplar_assign(d(boxes), n, d(ex), d(cnt), d(meta), max_ex, batch, m, thr, sa, si, sc)
    torch.cuda.synchronize()
    return sa.cpu().numpy(), si.cpu().numpy(), sc.cpu().numpy()


ASSIGN_CASES = [
    # n_anchor, batch, max_ex, m
    (1, 1, 1, 1), (1, 3, 16, 8), (84, 1, 1, 4), (84, 3, 16, 1), (84, 3, 16, 8), (255, 1, 16, 4), (256, 3, 1, 8), (257, 3, 16, 4),
    (257, 1, 1, 1), (8400, 3, 16, 4), (8400, 1, 16, 8), (8400, 1, 1, 1), (33600, 3, 16, 8), (33600, 1, 1, 4),
]


@pytest.mark.parametrize("n,batch,max_ex,m", ASSIGN_CASES, ids=[f"n{n}-b{b}-ex{x}-m{m}" for n, b, x, m in ASSIGN_CASES])
def test_assign_equals_the_reference_anchors_and_iou_bits(n, batch, max_ex, m):
    boxes, ex, cnt, meta = _case(n, batch, max_ex)
    for thr in (0.1, 0.0):
        a, i, c = _run_assign(boxes, ex, cnt, meta, m, thr)
        ra, ri, rc = R.assign(boxes, ex, cnt, meta, m, thr)
        assert np.array_equal(c, rc), (c, rc)
        bad = np.nonzero(a != ra)
        assert bad[0].size == 0, f"min_iou {thr}: anchors differ at {list(zip(*bad))[:5]}: {a[bad][:5]} vs {ra[bad][:5]}"
        assert np.array_equal(i.view(np.uint32), ri.view(np.uint32)), f"min_iou {thr}: IoU bits differ"
        # the sentinel slots: past ex_count, and the example that matches nothing
        rows = a.reshape(batch, max_ex, m)
        for b in range(batch):
            assert bool((rows[b, cnt[b]:] == -1).all()) and not i.reshape(batch, max_ex, m)[b, cnt[b]:].any()
            if cnt[b] > 3:
                assert bool((rows[b, 3] == -1).all())
    if n > 300 and m >= 4:                                                    # the duplicates tie at IoU 1, lower anchor first, across waves
        first = ra.reshape(batch, max_ex, m)[0, 0]
        assert first[:4].tolist() == [0, 1, 63, 64] and bool((ri.reshape(batch, max_ex, m)[0, 0, :4] == 1.0).all())


def test_assign_min_iou_boundary_and_nan_box_on_the_device():
    boxes = np.array([[[0, 0, 10, 10], [100, 100, 110, 110], [0, 0, 10, 10], [0, 0, 10, 20], [np.nan, 0, 10, 10], [0, 0, 20, 20]]], f32)
    ex = np.array([[[0, 0, 10, 10], [200, 200, 210, 210], [0, 0, 20, 20]]], f32)
    ident = np.array([[0, 0, 0, 1, 1, 64, 64, 0]], f32)
    for m, thr, cnt in ((4, 0.5, 3), (4, float(np.nextafter(f32(0.5), f32(0))), 3), (8, 0.0, 1), (2, 0.0, 0)):
        a, i, c = _run_assign(boxes, ex, np.array([cnt], np.int32), ident, m, thr)
        ra, ri, rc = R.assign(boxes, ex, [cnt], ident, m, thr)
        assert np.array_equal(a, ra) and np.array_equal(i.view(np.uint32), ri.view(np.uint32)) and np.array_equal(c, rc)
    a, _, _ = _run_assign(boxes, ex, np.array([3], np.int32), ident, 4, 0.5)
    assert a[0, :4].tolist() == [0, 2, -1, -1]                                # IoU == min_iou is not a candidate


# ------------------------------------------------------------------------------------------------------------------- pool
@functools.lru_cache(maxsize=None)
def _pool_inputs(dim: int = DIM, n_slot: int = 48):
    g = np.random.default_rng(77 + dim)
    emb = (g.standard_normal((3, n_slot, dim)) * np.exp(g.standard_normal((3, n_slot, 1)) * 2)).astype(f32)   # widely different norms
    anchors = g.integers(0, 84, n_slot).astype(np.int32)                      # levels mixed: offsets 64 / 80
    anchors[[0, 1, 2]] = [3, 70, 82]                                          # class 0 below holds all three levels
    anchors[[5, 17, 30]] = -1
    iou = (g.random(n_slot, dtype=f32) * 0.9 + 0.1).astype(f32)
    iou[anchors < 0] = 0
    classes = [list(range(0, 12)), [], [13], [5, 17, 30], [40, 3, 22, 3, 41, 42, 43, 44, 45, 46, 47, 20, 21, 23, 24, 25], [17, 31, 5, 32]]
    return emb, anchors, iou, classes


def _run_pool(emb, anchors, iou, classes, off1=64, off2=80):
    from wedetect_amd import exemplar as EX
    d = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    cls_off = np.cumsum([0] + [len(c) for c in classes]).astype(np.int32)
    cls_slot = np.array([s for c in classes for s in c] or [0], np.int32)
    bank = torch.full((len(classes), emb.shape[2]), float("nan"), dtype=torch.float32, device="cuda")
    sup = torch.full((len(classes),), -7, dtype=torch.int32, device="cuda")
    EX.exemplar_pool(d(emb), emb.shape[2], off1, off2, d(anchors), d(iou), emb.shape[1], d(cls_off), d(cls_slot), len(classes), bank, sup)
    torch.cuda.synchronize()
    return bank.cpu().numpy(), sup.cpu().numpy()


@pytest.mark.parametrize("dim", [768, 8, 1024])
def test_pool_against_float64_within_the_summation_bound(dim):
    emb, anchors, iou, classes = _pool_inputs(dim)
    bank, sup = _run_pool(emb, anchors, iou, classes)
    cls_off = np.cumsum([0] + [len(c) for c in classes])
    ref, rsup = R.pool(emb, 64, 80, anchors, iou, cls_off, [s for c in classes for s in c])
    assert sup.tolist() == rsup.tolist() == [12 - 1, 0, 1, 0, 16, 2]           # slot 5 of class 0 has no anchor; class 3 has none at all
    assert np.isfinite(bank).all()
    for c in range(len(classes)):
        err = float(np.abs(bank[c].astype(np.float64) - ref[c]).max())
        print(f"dim {dim} class {c}: rows {sup[c]}, max |d| {err:.3e}, bound {R.pool_bound(int(sup[c])):.3e}")
        assert err <= R.pool_bound(int(sup[c])), (c, err)
        if sup[c] == 0:
            assert not bank[c].any()                                          # the zero row of an empty class
        else:
            assert abs(float(np.linalg.norm(bank[c].astype(np.float64))) - 1) < 1e-6
    levels = R.level_of(anchors[classes[0]], 64, 80)
    assert len(set(levels[anchors[classes[0]] >= 0].tolist())) == 3           # levels mixed within one class
    # bit-identical on a second run
    bank2, sup2 = _run_pool(emb, anchors, iou, classes)
    assert np.array_equal(bank.view(np.uint32), bank2.view(np.uint32)) and np.array_equal(sup, sup2)
    # bit-identical with the class at another index and among a different number of classes
    for other, at in (([classes[4]], 0), ([[1, 2], classes[0], [], classes[4], [9], classes[5], [7, 8], classes[0]], None)):
        b3, s3 = _run_pool(emb, anchors, iou, other)
        if at is not None:
            assert np.array_equal(b3[at].view(np.uint32), bank[4].view(np.uint32)) and s3[at] == sup[4]
        else:
            for src, dst in ((0, 1), (4, 3), (5, 5), (0, 7)):
                assert np.array_equal(b3[dst].view(np.uint32), bank[src].view(np.uint32)) and s3[dst] == sup[src]


def test_pool_zero_and_non_finite_rows_give_a_zero_row():
    emb, anchors, iou, _ = _pool_inputs()
    emb = emb.copy()
    lv = R.level_of(anchors, 64, 80)
    emb[lv[0], 0] = 0                                                         # a zero row: 1 / sqrt(0) = inf, 0 * inf = NaN
    emb[lv[1], 1, 3] = np.inf
    bank, sup = _run_pool(emb, anchors, iou, [[0, 2], [1], [2]])
    assert sup.tolist() == [2, 1, 1] and not bank[0].any() and not bank[1].any() and bank[2].any() and np.isfinite(bank).all()
