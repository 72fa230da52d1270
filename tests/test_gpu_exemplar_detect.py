"""Exemplar prompts end to end (GPU): the ``nano`` model at 64 x 64 (84 anchors), built like the tiled-inference tests build it, in
fp16x3 and fp32 — the selected anchors' embeddings against ``ImageTower.embed`` bit for bit, self-retrieval, the bank used like a
text bank, pooling across the images of a batch, the range guard, the happens-before checker."""
import functools
import warnings

import numpy as np
import pytest
import torch

import tests.exemplar_hazards  # noqa: F401
from tests import exemplar_ref as R
from tests import hazards as H
from tests.test_gpu_tile import NAMES, _nano, _smooth_image

pytestmark = pytest.mark.gpu

f32 = np.float32
HW, B = 64, 2
# image 0 was never letterboxed; image 1: a 100 x 120 original at half scale, padded by 2 pixels left and 7 above
METAS = [dict(ori_shape=(HW, HW)), dict(ori_shape=(100, 120), scale_factor=(0.5, 0.5), pad_param=(7.0, 7.0, 2.0, 2.0))]
META_ROWS = np.array([[0, 0, 0, 1, 1, HW, HW, 1], [2, 7, 0, 0.5, 0.5, 120, 100, 1]], f32)
SELF_ANCHORS = (9, 37, 70, 82)                                                # two of level 0, one of level 1, one of level 2


def _inputs():
    from wedetect_amd.detector import DetDataSample
    xs = [torch.from_numpy(_smooth_image(HW, HW, seed=20 + b)).permute(2, 0, 1).contiguous() for b in range(B)]
    return xs, [DetDataSample(metainfo=dict(m)) for m in METAS]


@functools.lru_cache(maxsize=None)
def _world(precision):
    """(model, tower, decoded boxes [B, 84, 4] and region embeddings [B, 84, 768] of the batch on the host): the reference the tests
    share, computed once per arithmetic mode by one plain head."""
    from wedetect_amd.detector import _nhwc_u8
    m = _nano(precision)
    xs, _ = _inputs()
    x = _nhwc_u8(xs, m._h.device)
    tower = m._h.tower(B, HW, HW)
    m._h.calibrate_first(tower, x)
    embed, boxes = tower.features(x)
    torch.cuda.synchronize()
    assert tower.ntot == 84 and tower.off[1] == 64 and tower.off[2] == 80
    return m, tower, boxes.cpu().numpy().copy(), embed.cpu().numpy().copy()


def _to_original(box, b):
    mt = META_ROWS[b]
    return ((np.asarray(box, f32) - np.array([mt[0], mt[1]] * 2, f32)) / np.array([mt[3], mt[4]] * 2, f32)).astype(f32)


def _rows_of(tower):
    """The embedding rows the last exemplar_bank pooled from: [B * S, 768] by slot, from the level buffer of each slot's anchor."""
    ex = tower._ex
    anchors = ex["sel_anchors"].view(-1).cpu().numpy()
    t = ex["t"].cpu().numpy()
    lv = R.level_of(np.maximum(anchors, 0), tower.off[1], tower.off[2])
    return anchors, t[lv, np.arange(anchors.size)]


@pytest.mark.parametrize("precision", ["fp16x3", "fp32"])
def test_selected_embeddings_equal_the_tower_embed_bit_for_bit(precision):
    m, tower, boxes, embed = _world(precision)
    xs, samples = _inputs()
    # examples around decoded boxes of every level, pushed a little: each collects anchors of more than one level
    exemplars = [[(_to_original(boxes[b, a] + f32(d), b).tolist(), c) for c, (a, d) in enumerate(((5, 0.5), (66, -0.75), (81, 1.0), (40, 0.0)))]
                 for b in range(B)]
    bank, info = m.exemplar_bank(xs, samples, exemplars, anchors_per_box=8, min_iou=0.0)
    anchors, rows = _rows_of(tower)
    S = 4 * 8
    assert anchors.size == B * S and int((anchors >= 0).sum()) >= 40
    lv = R.level_of(anchors[anchors >= 0], 64, 80)
    assert set(lv.tolist()) == {0, 1, 2}, "the selection must reach every head level"
    for s, a in enumerate(anchors):
        if a >= 0:
            assert np.array_equal(rows[s].view(np.uint32), embed[s // S, a].view(np.uint32)), (s, a)
    # the assignment is the reference's on the decoded boxes, and [B, N, 768] materialised afterwards is the head's own
    ex = np.array([[bx for bx, _ in lst] for lst in exemplars], f32)
    ra, ri, _ = R.assign(boxes, ex, [4, 4], META_ROWS, 8, 0.0)
    assert np.array_equal(anchors.reshape(B, S), ra) and np.array_equal(tower._ex["sel_iou"].cpu().numpy().view(np.uint32), ri.view(np.uint32))
    assert np.array_equal(info["anchors"].numpy().reshape(B, S), ra)
    assert np.array_equal(tower.embed.cpu().numpy().view(np.uint32), embed.view(np.uint32))
    assert tuple(bank.shape) == (4, 768) and bank.is_cuda and info["support"] == [int((ra.reshape(B, 4, 8)[:, c] >= 0).sum()) for c in range(4)]


@pytest.mark.parametrize("precision", ["fp16x3", "fp32"])
def test_self_retrieval(precision):
    """An example box equal to the decoded box of anchor a with one anchor per box selects a; the prototype is embed[b, a]
    normalised.  Image 0 was never letterboxed, so its example is the decoded box itself and the IoU is exactly 1; image 1's box
    goes to original pixels and back — (x - pad) / scale, then x * scale + pad: up to four roundings per coordinate, each at most
    2^-24 of a value below 128, so a coordinate moves by less than 4e-5 pixels and the IoU of a box at least 0.2 pixels wide and
    high by less than 4 * 4e-5 / 0.2 = 8e-4: there the assertion is IoU > 0.999, and the anchor selected must still be a."""
    m, tower, boxes, embed = _world(precision)
    xs, samples = _inputs()
    exemplars = [[(_to_original(boxes[b, a], b).tolist(), c) for c, a in enumerate(SELF_ANCHORS)] for b in range(B)]
    names = [f"anchor {a}" for a in SELF_ANCHORS]
    for b in range(B):
        only = [exemplars[i] if i == b else [] for i in range(B)]
        bank, info = m.exemplar_bank(xs, samples, only, names, anchors_per_box=1, min_iou=0.1)
        assert info["support"] == [1] * 4 and info["names"] == names
        assert info["anchors"][b, :, 0].tolist() == list(SELF_ANCHORS), info["anchors"]
        if b == 0:
            assert info["ious"][b, :, 0].tolist() == [1.0] * 4
        else:
            assert float(info["ious"][b].min()) > 0.999
        assert bool((info["anchors"][1 - b] == -1).all())
        e64 = embed[b].astype(np.float64)
        cos = (bank.cpu().numpy().astype(np.float64) @ e64.T) / np.linalg.norm(e64, axis=1)[None, :]
        for c, a in enumerate(SELF_ANCHORS):
            print(f"{precision} image {b} anchor {a}: cosine {cos[c, a]:.9f}, best other {np.delete(cos[c], a).max():.6f}")
            assert abs(cos[c, a] - 1.0) <= R.pool_bound(1)
            assert float(np.delete(cos[c], a).max()) <= cos[c, a]


@pytest.mark.parametrize("precision", ["fp16x3", "fp32"])
def test_the_bank_is_used_like_a_text_bank(precision):
    m, tower, boxes, embed = _world(precision)
    xs, samples = _inputs()
    text_bank, texts = m.text_feats.clone(), m.texts
    exemplars = [[(_to_original(boxes[0, 9], 0).tolist(), 0), (_to_original(boxes[0, 70], 0).tolist(), 1)], [(_to_original(boxes[1, 30], 1).tolist(), 0)]]
    try:
        bank, info = m.set_exemplar_bank(xs, samples, exemplars, ["thing", "part"])
        assert m.texts == [["thing"], ["part"]] and torch.equal(m.text_feats, bank)
        p1 = [s.pred_instances for s in m.predict(*_inputs())]
        m.set_text_embeddings(bank.clone(), [["thing"], ["part"]])
        p2 = [s.pred_instances for s in m.predict(*_inputs())]
        assert sum(len(p.scores) for p in p1) >= 2
        for a, b in zip(p1, p2):
            for key in ("bboxes", "scores", "labels"):
                assert torch.equal(getattr(a, key), getattr(b, key)), key
        # text rows (any norm: normalised on the device) and prototypes (unit rows) in one bank, no per-image ``texts``
        k = text_bank.shape[0]
        m.set_text_embeddings(torch.cat([text_bank, bank]), [[n] for n in NAMES] + [["thing"], ["part"]])
        p3 = [s.pred_instances for s in m.predict(*_inputs())]
        labels = torch.cat([p.labels for p in p3])
        assert int(labels.max()) < k + 2 and bool((labels >= k).any()) and all(bool(torch.isfinite(p.scores).all()) for p in p3)
        # a class-aware step: the exemplar classes' rows of the mixed bank are the rows the exemplar-only bank gives
        for a, c in zip(p1, p3):
            keep = c.labels >= k
            if len(a.scores) < m._h.max_out and len(c.scores) < m._h.max_out:
                assert torch.equal(c.bboxes[keep], a.bboxes) and torch.equal(c.scores[keep], a.scores) and torch.equal(c.labels[keep] - k, a.labels)
    finally:
        m.set_text_embeddings(text_bank, texts)


@pytest.mark.parametrize("precision", ["fp16x3", "fp32"])
def test_one_class_from_two_images_equals_the_reference_pooling(precision):
    m, tower, boxes, embed = _world(precision)
    xs, samples = _inputs()
    exemplars = [[(_to_original(boxes[0, 20] + f32(0.5), 0).tolist(), 0)], [(_to_original(boxes[1, 75] - f32(0.5), 1).tolist(), 0), ((0.0, 0.0, 3.0, 3.0), 1)]]
    with pytest.raises(ValueError, match=r"class 1 \('nothing'\).*best IoU 0\.\d+"):
        m.exemplar_bank(xs, samples, exemplars, ["pair", "nothing"], anchors_per_box=4, min_iou=0.6)
    exemplars[1].pop()
    bank, info = m.exemplar_bank(xs, samples, exemplars, ["pair"], anchors_per_box=4, min_iou=0.05)
    anchors, ious = info["anchors"].numpy(), info["ious"].numpy()              # [B, 1, 4]
    ra, ri, _ = R.assign(boxes, np.array([[e[0][0]] for e in exemplars], f32), [1, 1], META_ROWS, 4, 0.05)
    assert np.array_equal(anchors.reshape(B, 4), ra) and np.array_equal(ious.reshape(B, 4).view(np.uint32), ri.view(np.uint32))
    assert int((ra >= 0).sum()) >= 5                                          # both images contribute, more than one anchor each
    lvl = np.zeros((3, B * 4, 768), f32)
    flat = ra.reshape(-1)
    for s, a in enumerate(flat):
        if a >= 0:
            lvl[int(R.level_of(a, 64, 80)), s] = embed[s // 4, a]
    ref, sup = R.pool(lvl, 64, 80, flat, ri.reshape(-1), [0, B * 4], list(range(B * 4)))
    err = float(np.abs(bank.cpu().numpy().astype(np.float64) - ref).max())
    print(f"{precision}: rows {int(sup[0])}, max |d| {err:.3e}, bound {R.pool_bound(int(sup[0])):.3e}")
    assert info["support"] == [int(sup[0])] and err <= R.pool_bound(int(sup[0]))


def test_range_guard_trip_yields_the_fp32_bank():
    """tests/test_gpu_feed.py's hot checkpoint, as the trip test of tests/test_gpu_views.py builds it: the fp16x3 build raises the
    range flag, the holder's fallback repeats it on the fp32 kernels, and the bank is the one an fp32 detector builds."""
    from tests.test_gpu_feed import _hot_state
    hot = _hot_state()
    m, m32 = _nano("fp16x3", hot, calibrate=False), _nano("fp32", hot, calibrate=False)
    xs, samples = _inputs()
    exemplars = [[((8.0, 8.0, 40.0, 40.0), 0), ((30.0, 20.0, 60.0, 50.0), 1)], [((20.0, 20.0, 90.0, 80.0), 0)]]
    with warnings.catch_warnings(record=True):
        warnings.simplefilter("always")
        bank, info = m.exemplar_bank(xs, samples, exemplars, min_iou=0.0)
    want, info32 = m32.exemplar_bank(xs, samples, exemplars, min_iou=0.0)
    t = m._h.tower(B, HW, HW)
    print(f"trips {t.fp16x3_trips} precision {t.precision} overflowed {t.overflowed}; support {info['support']}")
    assert t.fp16x3_trips >= 1 and t.precision == "fp32" and t.overflowed and m._h.precision == "fp32"
    assert bool(torch.isfinite(bank).all()) and min(info["support"]) >= 1
    assert info["support"] == info32["support"] and torch.equal(info["anchors"], info32["anchors"])
    assert torch.equal(bank, want)


def test_exemplar_bank_and_predict_are_ordered_for_the_happens_before_checker():
    m, tower, boxes, embed = _world("fp16x3")
    xs, samples = _inputs()
    exemplars = [[(_to_original(boxes[0, 9], 0).tolist(), 0)], [(_to_original(boxes[1, 70], 1).tolist(), 0)]]
    text_bank, texts = m.text_feats.clone(), m.texts
    m.exemplar_bank(xs, samples, exemplars)                                   # warm: lazily sized buffers exist, weights are split
    m.predict(*_inputs())
    torch.cuda.synchronize()
    from wedetect_amd.detector import _nhwc_u8
    x, meta = _nhwc_u8(xs, m._h.device), torch.from_numpy(META_ROWS).cuda()
    kw = dict(normalize_text=True, score_thr=0.001, nms="mmcv")
    plan_off, plan_slot = torch.tensor([0, 8], dtype=torch.int32).cuda(), torch.arange(8, dtype=torch.int32).cuda()
    ex_boxes = torch.tensor([[e[0][0]] for e in exemplars], dtype=torch.float32).cuda()
    ex_count = torch.ones(B, dtype=torch.int32).cuda()
    torch.cuda.synchronize()
    try:
        with H.track() as tr:
            m.set_exemplar_bank(xs, samples, exemplars, ["thing"])
            m.predict(*_inputs())
            # the tower's own calls around pipelined steps: the build reads c2 and the boxes a pending post-process may still use
            tower.detect(x, m.text_feats, meta, overlap_post=True, **kw)
            tower.exemplar_bank(x, meta, ex_boxes, ex_count, plan_off, plan_slot)
            tower.detect(x, m.text_feats, meta, overlap_post=True, **kw)
            tower.detect(x, m.text_feats, meta, **kw)
            tower.wait_post()
            torch.cuda.synchronize()
    finally:
        m.set_text_embeddings(text_bank, texts)
    assert tr.calls.get("exemplar.exemplar_assign", 0) == 2 and tr.calls.get("exemplar.exemplar_pool", 0) == 2
    assert tr.calls.get("fold.kept_rows_gather", 0) >= 2 and tr.calls.get("lib.nms_gather", 0) == 4
    assert len({s for _, s, _, _ in tr.model.launches}) >= 2, "everything ran on one stream: nothing was checked"
    hz = tr.hazards()
    assert hz == [], H.format_hazards(hz)
