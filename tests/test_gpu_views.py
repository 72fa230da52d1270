"""Test-time augmentation on the GPU (include/wedetect_hip_views.h, YOLOWorldDetector.predict_views): the flip against
``np.flip``, the merge against tests/views_ref.py (exact rows, labels, provenance, score and box bits), and the whole path on
the nano tower against views_ref fed by plain ``predict`` per view.  Every comparison is bit-identical."""
from __future__ import annotations

import numpy as np
import pytest
import torch

from tests import views_ref as R

pytestmark = pytest.mark.gpu

DEV = "cuda"


def _mods():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    from wedetect_amd import lib as L, views as VW
    return L, VW


# ------------------------------------------------------------------------------------------------------------------ flip
FLIP_SHAPES = [
    # (n, h, w), dst byte offset, what it exercises
    ((1, 1, 1), 0, "smallest"),
    ((2, 3, 5), 0, "byte path, odd w"),
    ((1, 4, 4), 0, "one vector"),
    ((1, 5, 7), 0, "byte path, odd w, misaligned rows"),
    ((3, 32, 33), 1, "dst at an odd address"),
    ((2, 64, 96), 0, "aligned dword path"),
]


@pytest.mark.parametrize("direction", [1, 2, 3], ids=["horizontal", "vertical", "diagonal"])
@pytest.mark.parametrize("shape,dst_off,what", FLIP_SHAPES, ids=[f"{s[0][0]}x{s[0][1]}x{s[0][2]} {s[2]}" for s in FLIP_SHAPES])
def test_flip_equals_numpy(shape, dst_off, what, direction):
    L, VW = _mods()
    n, h, w = shape
    img = np.random.default_rng(n * 1000 + h * 10 + w + direction).integers(0, 256, (n, h, w, 3), dtype=np.uint8)
    src = torch.from_numpy(img).to(DEV)
    nb = n * h * w * 3
    raw = torch.full((nb + 8,), 0xA5, dtype=torch.uint8, device=DEV)
    dst = raw[dst_off: dst_off + nb].view(n, h, w, 3)
    assert src.data_ptr() % 4 == 0 and dst.data_ptr() % 4 == dst_off % 4
    VW.flip_u8(src, dst, direction)
    torch.cuda.synchronize()
    want = R.flip(img, direction)
    got = dst.cpu().numpy()
    assert np.array_equal(got, want), f"{int((got != want).sum())} bytes differ"
    assert np.array_equal(src.cpu().numpy(), img)
    rest = torch.cat([raw[:dst_off], raw[dst_off + nb:]])
    assert bool((rest == 0xA5).all())
    if direction == 3:                                       # by name too
        VW.flip_u8(src, dst, "diagonal")
        torch.cuda.synchronize()
        assert np.array_equal(dst.cpu().numpy(), want)


def test_flip_twice_is_the_identity_and_overlap_is_refused():
    L, VW = _mods()
    img = torch.from_numpy(np.random.default_rng(5).integers(0, 256, (2, 9, 12, 3), dtype=np.uint8)).to(DEV)
    a, b = torch.empty_like(img), torch.empty_like(img)
    for d in (1, 2, 3):
        VW.flip_u8(img, a, d)
        VW.flip_u8(a, b, d)
        assert torch.equal(b, img)
    nb = img.numel()
    raw = torch.full((2 * nb,), 7, dtype=torch.uint8, device=DEV)
    call = lambda s, d, n=2, h=9, w=12, direction=1: VW.LIB.wd_flip_u8(s, d, n, h, w, direction, L.stream_ptr())
    p = raw.data_ptr()
    assert call(p, p) == -1 and call(p, p + nb - 1) == -1 and call(p + 1, p) == -1 and call(p + nb - 1, p) == -1
    assert call(p, p + nb, direction=0) == -1 and call(p, p + nb, direction=4) == -1 and call(p, p + nb, n=65536) == -1
    assert call(p, p + nb, h=0) == -1 and call(None, p) == -1
    torch.cuda.synchronize()
    assert bool((raw == 7).all())                            # nothing ran
    assert call(p, p + nb) == 0                              # adjacent ranges do not overlap
    torch.cuda.synchronize()


# ----------------------------------------------------------------------------------------------------------------- merge
def run_merge(c, n_cls, iou_thr, split_thr, max_out):
    L, VW = _mods()
    V, B, max_in = c["scores"].shape
    d = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    boxes, scores, labels, counts = d(c["boxes"]), d(c["scores"]), d(c["labels"]), d(c["counts"])
    vf, wh = d(c["view_flip"]), d(c["img_wh"])
    ws = torch.full((VW.merge_workspace_bytes(V, B, max_in),), 0xFF, dtype=torch.uint8, device=DEV)
    ob = torch.full((B, max_out, 4), float("nan"), device=DEV)
    os_ = torch.full((B, max_out), float("nan"), device=DEV)
    ol = torch.full((B, max_out), 12345, dtype=torch.int32, device=DEV)
    osrc = torch.full((B, max_out), 12345, dtype=torch.int32, device=DEV)
    oc = torch.full((B,), 12345, dtype=torch.int32, device=DEV)
    VW.views_merge(boxes, scores, labels, counts, vf, wh, V, B, max_in, n_cls, iou_thr, split_thr, max_out, ob, os_, ol, osrc, oc, ws)
    torch.cuda.synchronize()
    return dict(boxes=ob.cpu().numpy(), scores=os_.cpu().numpy(), labels=ol.cpu().numpy(), src=osrc.cpu().numpy(), count=oc.cpu().numpy())


def assert_merge_equal(got, want, images=None):
    sel = slice(None) if images is None else images
    assert np.array_equal(got["count"][sel], want["count"][sel]), (got["count"], want["count"])
    assert np.array_equal(got["src"][sel], want["src"][sel]), "provenance differs"
    assert np.array_equal(got["labels"][sel], want["labels"][sel])
    assert np.array_equal(got["scores"][sel].view(np.uint32), want["scores"][sel].view(np.uint32)), "score bits differ"
    assert np.array_equal(got["boxes"][sel].view(np.uint32), want["boxes"][sel].view(np.uint32)), "box bits differ"


IOU = 0.5
MERGE_CASES = [
    # id, V, B, max_in, counts, flips, n_cls, split_thr, max_out
    ("1x1x5 smallest", 1, 1, 5, "full", [0], 1, 10000, 300),
    ("2x1x8: 16 keys", 2, 1, 8, "full", [1, 0], 80, 10000, 300),
    ("2x3x300 the shipped shape", 2, 3, 300, "mixed", [1, 0], 80, 10000, 300),
    ("2x33x300 LVIS offsets", 2, 33, 300, "mixed", [1, 0], 1203, 10000, 100),
    ("4x2x64 all flip codes, per class, max_out 7", 4, 2, 64, "mixed", [0, 1, 2, 3], 80, 8, 7),
    ("8x2x512 both caps", 8, 2, 512, "full", [0, 1, 2, 3, 1, 0, 3, 2], 80, 10000, 1024),
]
_WANT = {}


def _case(name, V, B, max_in, counts, flips, n_cls, split_thr, max_out):
    """Inputs and reference of a case, computed once and shared (never modified)."""
    if name not in _WANT:
        c = R.merge_inputs(V, B, max_in, seed=V * 100 + B, counts=counts, flips=flips, n_cls=n_cls)
        _WANT[name] = (c, R.merge(c["boxes"], c["scores"], c["labels"], c["counts"], c["view_flip"], c["img_wh"], n_cls, IOU, split_thr, max_out))
    return _WANT[name]


@pytest.mark.parametrize("name,V,B,max_in,counts,flips,n_cls,split_thr,max_out", MERGE_CASES, ids=[c[0] for c in MERGE_CASES])
def test_merge_equals_reference(name, V, B, max_in, counts, flips, n_cls, split_thr, max_out):
    c, want = _case(name, V, B, max_in, counts, flips, n_cls, split_thr, max_out)
    # what the case exercises, shown by the reference alone
    assert bool((c["img_wh"] % 2 == 1).all())                # odd image sizes
    assert int(want["count"].max()) >= 1
    if V > 1:
        assert int(((want["per_view"] > 0).sum(1) >= 2).sum()) >= 1          # rows of at least two views survive in one image
        assert int(want["cross_view"].sum()) >= 1                          # a row is suppressed by a row of ANOTHER view
    if counts == "mixed":
        assert 0 in c["counts"] and max_in in c["counts"] and bool(((c["counts"] > 0) & (c["counts"] < max_in)).any())
    if max_out == 7:
        assert bool((want["count"] == 7).all())              # truncation
        assert bool((c["counts"].clip(0).sum(0) >= split_thr).all())         # the per-class branch
    got = run_merge(c, n_cls, IOU, split_thr, max_out)
    print(f"{name}: rows {want['count'].tolist()[:8]}, per view {want['per_view'].tolist()[:3]}, cross-view suppressions "
          f"{want['cross_view'].tolist()[:8]}")
    assert_merge_equal(got, want)


def test_merge_planted_mirrored_pair():
    """One object seen by the flipped view (score 0.9) and, mirrored, by the plain view (0.8): the flipped view's row stays."""
    W, H = 641.0, 427.0
    c = dict(boxes=np.zeros((2, 1, 4, 4), np.float32), scores=np.zeros((2, 1, 4), np.float32), labels=np.zeros((2, 1, 4), np.int32),
             counts=np.asarray([[1], [2]], np.int32), view_flip=np.asarray([1, 0], np.int32), img_wh=np.asarray([[W, H]], np.float32))
    c["boxes"][0, 0, 0] = (W - 110.25, 50, W - 10.5, 90)     # the flipped view sees (10.5, 50, 110.25, 90) mirrored
    c["scores"][0, 0, 0] = 0.9
    c["boxes"][1, 0, :2] = [(10.5, 50, 110.25, 90), (300, 300, 340, 360)]
    c["scores"][1, 0, :2] = (0.8, 0.5)
    got = run_merge(c, 80, 0.5, 10000, 100)
    assert got["count"].tolist() == [2] and got["src"][0, :2].tolist() == [0, 5]
    assert got["boxes"][0, 0].tolist() == [10.5, 50, 110.25, 90] and got["scores"][0, :2].tolist() == [float(np.float32(0.9)), 0.5]
    want = R.merge(c["boxes"], c["scores"], c["labels"], c["counts"], c["view_flip"], c["img_wh"], 80, 0.5, 10000, 100)
    assert want["cross_view"].tolist() == [1]
    assert_merge_equal(got, want)


def test_merge_all_counts_zero_writes_every_row():
    c = R.merge_inputs(2, 3, 64, seed=1, counts="zero")
    got = run_merge(c, 80, 0.5, 10000, 300)
    assert not got["count"].any() and not got["boxes"].any() and not got["scores"].any()
    assert bool((got["labels"] == -1).all()) and bool((got["src"] == -1).all())


def test_merge_guard_is_per_image():
    """One view of ONE image reports -1: that image alone gives -1 (rows all filler); the others are bit-identical."""
    name = MERGE_CASES[2][0]
    c, want = _case(*MERGE_CASES[2])
    clean = run_merge(c, 80, IOU, 10000, 300)
    bad = dict(c, counts=c["counts"].copy())
    bad["counts"][1, 0] = -1
    got = run_merge(bad, 80, IOU, 10000, 300)
    assert got["count"][0] == -1 and not got["boxes"][0].any() and not got["scores"][0].any()
    assert bool((got["labels"][0] == -1).all()) and bool((got["src"][0] == -1).all())
    assert_merge_equal(got, clean, images=slice(1, None))
    assert_merge_equal(got, R.merge(bad["boxes"], bad["scores"], bad["labels"], bad["counts"], bad["view_flip"], bad["img_wh"], 80, IOU,
                                    10000, 300, witness=False))
    assert name in _WANT


def test_merge_refuses_what_is_over_the_cap():
    L, VW = _mods()
    z = torch.zeros(64, dtype=torch.float32, device=DEV)
    ws = torch.zeros(1 << 21, dtype=torch.uint8, device=DEV)
    out = torch.full((16,), 5, dtype=torch.int32, device=DEV)

    def call(V, B, max_in, n_cls, max_out, thr=0.5):
        p = z.data_ptr()
        return VW.LIB.wd_views_merge(p, p, p, p, p, p, V, B, max_in, n_cls, thr, 10000, max_out, p, p, out.data_ptr(), out.data_ptr(),
                                     out.data_ptr(), ws.data_ptr(), ws.numel(), L.stream_ptr())
    assert call(9, 1, 4, 80, 300) == -4 and call(0, 1, 4, 80, 300) == -4        # views outside 1 .. 8
    assert call(8, 1, 513, 80, 300) == -4 and call(2, 1, 2049, 80, 300) == -4    # one over V * max_in = 4096
    assert call(2, 1, 300, 80, 1025) == -4
    assert call(8, 1, 512, 1 << 19, 300) == -4               # 4096 * 2^19 = 2^31
    assert call(2, 65536, 4, 80, 300) == -1 and call(2, 1, 0, 80, 300) == -1 and call(2, 1, 4, 80, 300, float("nan")) == -1
    assert VW.merge_workspace_bytes(9, 1, 4) == 0 == VW.merge_workspace_bytes(8, 1, 513) < VW.merge_workspace_bytes(8, 1, 512)
    assert VW.LIB.wd_views_merge(z.data_ptr(), z.data_ptr(), z.data_ptr(), z.data_ptr(), z.data_ptr(), z.data_ptr(), 2, 1, 4, 80, 0.5,
                                 10000, 8, z.data_ptr(), z.data_ptr(), out.data_ptr(), out.data_ptr(), out.data_ptr(), ws.data_ptr(), 256,
                                 L.stream_ptr()) == -3       # workspace too small
    torch.cuda.synchronize()
    assert bool((out == 5).all())                            # nothing ran


# ------------------------------------------------------------------------------------------------------------ end to end
from tests.test_gpu_tile import NAMES, _nano, _smooth_image  # noqa: E402

TTA_CFG = dict(nms=dict(type="nms", iou_threshold=0.5), max_per_img=100)
META_KEYS = ("img_id", "ori_shape", "img_shape", "scale_factor", "pad_param", "texts", "flip", "flip_direction")
SIZES = [(50, 61), (64, 47), (39, 64)]                       # (h, w) of the images: odd sides, odd total pads at 64 and at 96


def _tta_pipeline(scales, directions=("horizontal",)):
    """mmyolo's TTA pipeline shape: resize branches x flip branches x PackDetInputs."""
    from wedetect_amd import tta  # noqa: F401  (registers TestTimeAug / RandomFlip: this file also runs on its own)
    from wedetect_amd.pipeline import Compose
    resize = [dict(type="Compose", transforms=[dict(type="WeDetectKeepRatioResize", scale=(s, s)),
                                               dict(type="WeDetectLetterResize", scale=(s, s), allow_scale_up=False, pad_val=dict(img=114))])
              for s in scales]
    flips = [dict(type="RandomFlip", prob=1.0, direction=d) for d in directions] + [dict(type="RandomFlip", prob=0.0)]
    return Compose([dict(type="LoadImageFromFile"), dict(type="LoadText"),
                    dict(type="TestTimeAug", transforms=[resize, flips, [dict(type="PackDetInputs", meta_keys=META_KEYS)]])])


def _items(pipe, n, texts=None, seed=11):
    out = []
    for i in range(n):
        h, w = SIZES[i % len(SIZES)]
        bgr = np.ascontiguousarray(_smooth_image(h, w, seed + i)[:, :, ::-1])
        out.append(pipe(dict(img=bgr, img_id=i, texts=(texts[i] if texts is not None else [[n_] for n_ in NAMES]))))
    return out


def _views_of(items):
    from wedetect_amd.tta import collate_views
    data = collate_views(items)
    return list(zip(data["inputs"], data["data_samples"])), data


def _fresh(views):
    """The same views with samples of their own (``predict`` / ``predict_views`` attach their results to the samples)."""
    return [(x, [type(s)(metainfo=s.metainfo) for s in samples]) for x, samples in views]


def _assert_samples_equal(got, want, max_in):
    assert len(got) == len(want["count"])
    for b, s in enumerate(got):
        p = s.pred_instances
        n = int(want["count"][b])
        assert len(p.scores) == n, (b, len(p.scores), n)
        assert not p.bboxes.is_cuda
        assert torch.equal(p.bboxes, torch.from_numpy(want["boxes"][b, :n])), b
        assert torch.equal(p.scores, torch.from_numpy(want["scores"][b, :n])), b
        assert torch.equal(p.labels, torch.from_numpy(want["labels"][b, :n]).to(torch.int64)), b
        assert torch.equal(p.views, torch.from_numpy(want["src"][b, :n] // max_in).to(torch.int64)), b


def _witnesses(want, V):
    assert int(want["count"].min()) >= 1
    if V > 1:
        assert int(((want["per_view"] > 0).sum(1) >= 2).sum()) >= 1      # rows of at least two views survive in one image
        assert int(want["cross_view"].sum()) >= 1                      # a row is suppressed by a row of ANOTHER view


E2E = [("flip + plain at 64, B = 3", (64,), 3, False), ("two scales x flip, B = 2", (64, 96), 2, False),
       ("flip + plain, two class lists in the batch", (64,), 3, True)]


@pytest.mark.parametrize("precision", ["fp32", "fp16x3"])
@pytest.mark.parametrize("name,scales,B,two_lists", E2E, ids=[e[0] for e in E2E])
def test_predict_views_equals_the_user_route(name, scales, B, two_lists, precision):
    from wedetect_amd import weights as W
    m_ref, m = _nano(precision), _nano(precision)
    texts = None
    if two_lists:
        bank = torch.from_numpy(W.make_text_bank(len(NAMES))).cuda()
        short = [[n] for n in NAMES[3:12]]
        for mm in (m_ref, m):
            mm._banks[tuple(t[0] for t in short)] = bank[3:12].clone()
        texts = [[[n] for n in NAMES], short, [[n] for n in NAMES]]
    views, _ = _views_of(_items(_tta_pipeline(scales), B, texts))
    V = 2 * len(scales)
    assert len(views) == V and [tuple(x.shape[-2:]) for x, _ in views] == [(s, s) for s in scales for _ in range(2)]
    assert [s[0].metainfo["flip"] for _, s in views] == [True, False] * len(scales)
    assert any(float(s.metainfo["pad_param"][:2].sum()) % 2 == 1 or float(s.metainfo["pad_param"][2:].sum()) % 2 == 1
               for s in views[0][1])                         # an odd total pad: the reproduced one-pixel asymmetry is in play
    want = R.user_route(m_ref, _fresh(views), TTA_CFG)
    stats = {}
    got = m.predict_views(_fresh(views), TTA_CFG, stats=stats)
    print(f"{name} {precision}: rows in {want['per_view_in'].tolist()}, merged {want['count'].tolist()}, per view "
          f"{want['per_view'].tolist()}, cross-view suppressions {want['cross_view'].tolist()}; stats {stats}")
    _witnesses(want, V)
    assert stats == dict(views=V, steps=V, trips=0, inline=False, d2h_copies=1)
    _assert_samples_equal(got, want, m._h.max_out)
    for b, s in enumerate(got):                              # the FIRST view's sample
        assert s.metainfo["flip"] is True and s.metainfo["img_id"] == b
    if two_lists:
        assert int(got[1].pred_instances.labels.max()) < 9
    # a second call on the cached buffers: the same rows
    _assert_samples_equal(m.predict_views(_fresh(views), TTA_CFG), want, m._h.max_out)


def test_predict_views_all_flip_directions_and_empty_images():
    m_ref, m = _nano("fp16x3"), _nano("fp16x3")
    views, _ = _views_of(_items(_tta_pipeline((64,), ("horizontal", "vertical", "diagonal")), 2))
    assert [s[0].metainfo["flip_direction"] for _, s in views] == ["horizontal", "vertical", "diagonal", None]
    want = R.user_route(m_ref, _fresh(views), TTA_CFG)
    _witnesses(want, 4)
    _assert_samples_equal(m.predict_views(_fresh(views), TTA_CFG), want, m._h.max_out)
    # no row passes the score threshold: empty instances
    m.test_cfg["score_thr"] = 2.0
    for s in m.predict_views(_fresh(views), TTA_CFG):
        p = s.pred_instances
        assert len(p.scores) == 0 and tuple(p.bboxes.shape) == (0, 4) and len(p.labels) == 0 and len(p.views) == 0
    # a view whose samples disagree about the flip; more than 8 views
    bad = _fresh(views)
    bad[0][1][1].set_metainfo(dict(flip=False, flip_direction=None))
    with pytest.raises(ValueError):
        m.predict_views(bad, TTA_CFG)
    with pytest.raises(NotImplementedError):
        m.predict_views(_fresh(views) * 3, TTA_CFG)


def test_det_tta_model_test_step_on_a_pipelines_output_equals_predict_views():
    from wedetect_amd.registry import MODELS
    m_a, m_b = _nano("fp16x3"), _nano("fp16x3")
    items = _items(_tta_pipeline((64,)), 3)
    views, data = _views_of(items)
    want = m_a.predict_views(_fresh(views), TTA_CFG)
    tta = MODELS.build(dict(type="DetTTAModel", tta_cfg=TTA_CFG, module=m_b))
    stats = {}
    got = tta.test_step(data, stats=stats)                   # what the pipeline + collate produced, as it is
    assert stats["d2h_copies"] == 1 and len(got) == 3 and int(sum(len(s.pred_instances.scores) for s in want)) >= 3
    for a, b in zip(want, got):
        for key in ("bboxes", "scores", "labels", "views"):
            assert torch.equal(getattr(a.pred_instances, key), getattr(b.pred_instances, key)), key


def test_predict_views_range_guard_trip_equals_the_in_line_result():
    """tests/test_gpu_feed.py's hot checkpoint: the pipelined steps only detect the trip; the views then run one by one in line
    through ``checked_counts`` and give what ``predict`` per view gives, tower state included."""
    import warnings
    from tests.test_gpu_feed import _hot_state
    hot = _hot_state()
    m_ref, m = _nano("fp16x3", hot, calibrate=False), _nano("fp16x3", hot, calibrate=False)
    views, _ = _views_of(_items(_tta_pipeline((64,)), 3))
    with warnings.catch_warnings(record=True):
        warnings.simplefilter("always")
        want = R.user_route(m_ref, _fresh(views), TTA_CFG)
        stats = {}
        got = m.predict_views(_fresh(views), TTA_CFG, stats=stats)
    t_a, t_b = m_ref._h.tower(3, 64, 64), m._h.tower(3, 64, 64)
    print(f"trip: stats {stats}; in-line trips {t_a.fp16x3_trips} precision {t_a.precision}; views trips {t_b.fp16x3_trips} "
          f"precision {t_b.precision}; merged {want['count'].tolist()}")
    assert stats["trips"] == 1 and stats["inline"] and stats["d2h_copies"] == 2 and t_a.fp16x3_trips >= 1
    assert t_b.fp16x3_trips == t_a.fp16x3_trips and t_b.precision == t_a.precision and t_b.overflowed == t_a.overflowed
    assert int(want["count"].min()) >= 1
    _assert_samples_equal(got, want, m._h.max_out)
    # while the tower is in its fallback every step goes in line, as the in-line route does
    want2 = R.user_route(m_ref, _fresh(views), TTA_CFG)
    stats = {}
    got2 = m.predict_views(_fresh(views), TTA_CFG, stats=stats)
    assert stats["inline"] and stats["trips"] == 0 and stats["d2h_copies"] == 1
    _assert_samples_equal(got2, want2, m._h.max_out)
