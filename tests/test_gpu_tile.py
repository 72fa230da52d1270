"""Tiled inference on the GPU (include/wedetect_hip_tile.h, YOLOWorldDetector.predict_tiled): the cut against numpy slicing, the
merge against tests/tile_ref.py (exact rows, labels, provenance, score bits), and the whole path on the nano tower against
tile_ref fed by plain ``predict`` on host-cut tiles in the same groups."""
from __future__ import annotations

import numpy as np
import pytest
import torch

from tests import tile_ref as R

pytestmark = pytest.mark.gpu

DEV = "cuda"


def _mods():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    from wedetect_amd import lib as L, tile as T, tiling as G
    return L, T, G


def _image(h, w, seed=0):
    return np.random.default_rng(seed).integers(0, 256, (h, w, 3), dtype=np.uint8)


# ------------------------------------------------------------------------------------------------------------------- cut
CUT_CASES = [
    # id, image (h, w), tile, overlap, padded pitch, swap_rb, dst offset, extra
    ("70x101 tile 32 dense", (70, 101), (32, 32), 0.25, 0, 0, 0, None),
    ("70x101 tile 32 pitch+5 swapped", (70, 101), (32, 32), 0.25, 5, 1, 0, None),
    ("70x101 tile 64x96 shifted last tile", (70, 101), (64, 96), 0.2, 0, 0, 0, None),
    ("70x101 tile 64x96 pitch+13 dst odd", (70, 101), (64, 96), 0.2, 13, 1, 1, None),
    ("20x50 in 32x64 (fill)", (20, 50), (32, 64), 0.2, 0, 0, 0, None),
    ("20x50 in 32x64 swapped dst odd", (20, 50), (32, 64), 0.2, 3, 1, 3, None),
    ("70x101 tile 32 + blank + overview untouched", (70, 101), (32, 32), 0.25, 7, 0, 0, "blank"),
]


@pytest.mark.parametrize("name,hw,tile,overlap,pad,swap,dst_off,extra", CUT_CASES, ids=[c[0] for c in CUT_CASES])
def test_cut_equals_numpy_slicing(name, hw, tile, overlap, pad, swap, dst_off, extra):
    L, T, G = _mods()
    h, w = hw
    img = _image(h, w, seed=h + w + pad)
    plan = G.plan_tiles(h, w, tile, overlap, overview=extra is not None)
    if extra == "blank":
        plan = G.pad_plan(plan, len(plan) + 2)
        assert (plan["kind"] == G.OVERVIEW).sum() == 1 and (plan["kind"] == G.BLANK).sum() == 2
    if hw == (70, 101) and tile == (64, 96):
        assert plan["x0"].tolist()[:2] == [0, 5] and plan["y0"].tolist()[-1] == 6            # the last tiles are shifted inward
    n, (th, tw) = len(plan), tile
    pitch = w * 3 + pad
    host = np.full((h, pitch), 0xEE, np.uint8)               # the bytes between two rows are no pixels
    host[:, : w * 3] = img.reshape(h, w * 3)
    src = torch.from_numpy(host).to(DEV)
    view = torch.as_strided(src, (h, w, 3), (pitch, 3, 1))
    plan_dev = torch.from_numpy(plan.view(np.uint8).copy()).to(DEV)
    raw = torch.full((n * th * tw * 3 + 8,), 0xA5, dtype=torch.uint8, device=DEV)
    dst = raw[dst_off: dst_off + n * th * tw * 3].view(n, th, tw, 3)
    assert dst.data_ptr() % 4 == dst_off % 4
    T.tile_cut_u8(view, plan_dev.data_ptr(), plan, dst, fill=114, swap_rb=bool(swap))
    torch.cuda.synchronize()
    want = R.cut(img, plan, tile, 114, bool(swap), dst=np.full((n, th, tw, 3), 0xA5, np.uint8))
    got = dst.cpu().numpy()
    assert np.array_equal(got, want), f"{int((got != want).sum())} bytes differ"
    assert torch.equal(dst.cpu(), torch.from_numpy(want))
    rest = torch.cat([raw[:dst_off], raw[dst_off + n * th * tw * 3:]])
    assert bool((rest == 0xA5).all())
    if extra == "blank":
        k = int(np.nonzero(plan["kind"] == G.OVERVIEW)[0][0])
        assert bool((dst[k] == 0xA5).all())                  # the overview slot keeps its pattern
        assert bool((dst[-1] == 114).all())


def test_cut_refuses_windows_outside_the_image():
    L, T, G = _mods()
    img = torch.from_numpy(_image(40, 50)).to(DEV)
    plan = G.plan_tiles(40, 50, (32, 32), 0.25, overview=False)
    dst = torch.full((len(plan), 32, 32, 3), 7, dtype=torch.uint8, device=DEV)
    dev = torch.from_numpy(plan.view(np.uint8).copy()).to(DEV)
    for field, v in (("x0", 19), ("y0", -1), ("w", 33), ("h", 0), ("kind", 3)):
        bad = plan.copy()
        bad[field][len(plan) - 1] = v
        rc = T.LIB.wd_tile_cut_u8(img.data_ptr(), 40, 50, 150, dev.data_ptr(), bad.ctypes.data, len(plan), 32, 32, 114, 0, dst.data_ptr(),
                                  L.stream_ptr())
        assert rc == -1, (field, rc)
    assert T.LIB.wd_tile_cut_u8(img.data_ptr(), 40, 50, 149, dev.data_ptr(), plan.ctypes.data, len(plan), 32, 32, 114, 0, dst.data_ptr(),
                                L.stream_ptr()) == -1
    torch.cuda.synchronize()
    assert bool((dst == 7).all())                            # nothing ran


# ----------------------------------------------------------------------------------------------------------------- merge
def run_merge(c, n_cls, edge_margin, iou_thr, split_thr, max_out):
    L, T, G = _mods()
    n_tile, max_in = c["scores"].shape
    d = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    boxes, scores, labels, counts = d(c["boxes"]), d(c["scores"]), d(c["labels"]), d(c["counts"])
    plan_dev = d(c["plan"].view(np.uint8).copy())
    ws = torch.full((T.merge_workspace_bytes(n_tile, max_in),), 0xFF, dtype=torch.uint8, device=DEV)
    ob = torch.full((max_out, 4), float("nan"), device=DEV)
    os_ = torch.full((max_out,), float("nan"), device=DEV)
    ol = torch.full((max_out,), 12345, dtype=torch.int32, device=DEV)
    osrc = torch.full((max_out,), 12345, dtype=torch.int32, device=DEV)
    oc = torch.full((1,), 12345, dtype=torch.int32, device=DEV)
    T.tile_merge(boxes, scores, labels, counts, plan_dev.data_ptr(), n_tile, max_in, n_cls, edge_margin, iou_thr, split_thr, max_out,
                 ob, os_, ol, osrc, oc, ws)
    torch.cuda.synchronize()
    return dict(boxes=ob.cpu().numpy(), scores=os_.cpu().numpy(), labels=ol.cpu().numpy(), src=osrc.cpu().numpy(), count=int(oc.item()))


def assert_merge_equal(got, want):
    assert got["count"] == want["count"], (got["count"], want["count"])
    assert np.array_equal(got["src"], want["src"]), "provenance differs"
    assert np.array_equal(got["labels"], want["labels"])
    assert np.array_equal(got["scores"].view(np.uint32), want["scores"].view(np.uint32)), "score bits differ"
    assert np.array_equal(got["boxes"].view(np.uint32), want["boxes"].view(np.uint32)), "box bits differ"


MERGE_CASES = [
    # id, n_tile, max_in, counts, edge_margin, split_thr, max_out
    ("1x5", 1, 5, "mixed", 0.0, 10000, 300),
    ("3x64 margin 2", 3, 64, "mixed", 2.0, 10000, 300),
    ("3x64 full counts margin 0", 3, 64, "full", 0.0, 10000, 300),
    ("9x300 margin 2 per class (split_thr 8)", 9, 300, "mixed", 2.0, 8, 300),
    ("9x300 margin 0 max_out 7", 9, 300, "mixed", 0.0, 10000, 7),
    ("128x256 the cap, margin 2", 128, 256, "mixed", 2.0, 10000, 1024),
]


@pytest.mark.parametrize("name,n_tile,max_in,counts,margin,split_thr,max_out", MERGE_CASES, ids=[c[0] for c in MERGE_CASES])
def test_merge_equals_reference(name, n_tile, max_in, counts, margin, split_thr, max_out):
    c = R.merge_inputs(n_tile, max_in, seed=n_tile, counts=counts)
    want = R.merge(c["boxes"], c["scores"], c["labels"], c["counts"], c["plan"], R.N_CLS, margin, 0.7, split_thr, max_out)
    # what the case exercises, shown by the reference alone
    if n_tile > 1:                                           # one tile has no other tile to be suppressed by
        assert want["cross_tile"] >= 1
    if margin > 0:
        assert want["dropped"] >= 1
    assert want["count"] >= 1
    if max_out == 7:
        full = R.merge(c["boxes"], c["scores"], c["labels"], c["counts"], c["plan"], R.N_CLS, margin, 0.7, split_thr, 1024)
        assert full["count"] > 7 == want["count"]
    if n_tile >= 3:
        k = want["count"]
        assert 1202 in want["labels"][:k].tolist()
        assert bool((want["scores"][1:k] == want["scores"][:k - 1]).any())       # equal scores: the slot decides
        assert len(set((want["src"][:k] // max_in).tolist())) > 1                # rows of several tiles
    got = run_merge(c, R.N_CLS, margin, 0.7, split_thr, max_out)
    print(f"{name}: {want['count']} rows, {want['dropped']} border drops, {want['cross_tile']} cross-tile suppressions")
    assert_merge_equal(got, want)


def test_merge_planted_pairs_across_an_overlap():
    """The object both crops of an overlap see keeps its higher-scoring row only; the pair of IoU 0.6 keeps both."""
    c = R.merge_inputs(3, 64, seed=3)
    got = run_merge(c, R.N_CLS, 2.0, 0.7, 10000, 300)
    kept = set(got["src"][:got["count"]].tolist())
    find = lambda t, s: int(t * 64 + np.nonzero(c["scores"][t, :c["counts"][t]] == np.float32(s))[0][0])
    assert find(0, 0.9140625) in kept and find(1, 0.8828125) not in kept
    assert find(0, 0.8515625) in kept and find(1, 0.8203125) in kept
    assert find(2, 0.9765625) in kept and find(0, 0.9453125) not in kept              # the overview's row wins over crop 0's


def test_merge_all_counts_zero_writes_every_row():
    c = R.merge_inputs(3, 64, seed=1, counts="zero")
    got = run_merge(c, R.N_CLS, 2.0, 0.7, 10000, 300)
    assert got["count"] == 0 and not got["boxes"].any() and not got["scores"].any()
    assert bool((got["labels"] == -1).all()) and bool((got["src"] == -1).all())


def test_merge_reports_a_tile_that_tripped():
    c = R.merge_inputs(9, 300, seed=9)
    c["counts"][3] = -1
    want = R.merge(c["boxes"], c["scores"], c["labels"], c["counts"], c["plan"], R.N_CLS, 2.0, 0.7, 10000, 300)
    got = run_merge(c, R.N_CLS, 2.0, 0.7, 10000, 300)
    assert want["count"] == -1 == got["count"]
    assert_merge_equal(got, want)
    # a blank tile's count is not read: -1 there is no trip
    c = R.merge_inputs(128, 256, seed=128)
    c["counts"][127] = -1
    assert c["plan"][127]["kind"] == R.BLANK
    assert run_merge(c, R.N_CLS, 2.0, 0.7, 10000, 1024)["count"] == 1024


def test_merge_refuses_what_is_over_the_cap():
    L, T, G = _mods()
    z = torch.zeros(64, dtype=torch.float32, device=DEV)
    ws = torch.zeros(1 << 21, dtype=torch.uint8, device=DEV)
    out = torch.full((16,), 5, dtype=torch.int32, device=DEV)

    def call(n_tile, max_in, n_cls, max_out):
        return T.LIB.wd_tile_merge(z.data_ptr(), z.data_ptr(), z.data_ptr(), z.data_ptr(), z.data_ptr(), n_tile, max_in, n_cls, 2.0, 0.7,
                                   10000, max_out, z.data_ptr(), z.data_ptr(), out.data_ptr(), out.data_ptr(), out.data_ptr(),
                                   ws.data_ptr(), ws.numel(), L.stream_ptr())
    assert call(128, 257, 80, 300) == -4 and call(129, 256, 80, 300) == -4      # one over n_tile * max_in = 32768
    assert call(9, 300, 80, 1025) == -4
    assert call(128, 256, 65536, 300) == -4                  # 32768 * 65536 = 2^31
    assert T.merge_workspace_bytes(129, 256) == 0 < T.merge_workspace_bytes(128, 256)
    torch.cuda.synchronize()
    assert bool((out == 5).all())                            # nothing ran


# ------------------------------------------------------------------------------------------------------------ end to end
NAMES = [f"class {k}" for k in range(20)]
TILE = (64, 64)
_SD = {}


def _smooth_image(h, w, seed):
    """Smooth content + a little noise (tests/test_gpu_feed.py's recipe), RGB."""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float32)
    chans = []
    for c in range(3):
        fx, fy, ph = rng.uniform(0.05, 0.3), rng.uniform(0.05, 0.3), rng.uniform(0, 6.28)
        chans.append(127 + 90 * np.sin(fx * xx + ph) * np.cos(fy * yy + c) + rng.normal(0, 12, (h, w)))
    return np.clip(np.stack(chans, -1), 0, 255).astype(np.uint8)


def _nano(precision, state=None, calibrate=True):
    from wedetect_amd import weights as W
    from wedetect_amd.detector import YOLOWorldDetector
    if "nano" not in _SD:
        _SD["nano"] = {k: torch.from_numpy(v) for k, v in W.make_state_dict("nano").items()}
    m = YOLOWorldDetector("nano", test_cfg=dict(max_per_img=100), max_classes=len(NAMES), precision=precision)
    m.load_state_dict(state if state is not None else _SD["nano"])
    m.cuda().eval()
    m._h.auto_calibrate = calibrate
    m.set_text_embeddings(torch.from_numpy(W.make_text_bank(len(NAMES))).cuda(), [[n] for n in NAMES])
    return m


_pipeline_canvas = R.pipeline_canvas


def _user_route(model, img_rgb, tile, overlap, overview, tile_batch, edge_margin):
    return R.user_route(model, img_rgb, tile, overlap, overview, tile_batch, edge_margin, len(NAMES))


def _assert_sample_equals(sample, want):
    p = sample.pred_instances
    n = want["count"]
    assert len(p.scores) == n
    assert torch.equal(p.bboxes.cpu(), torch.from_numpy(want["boxes"][:n]))
    assert torch.equal(p.scores.cpu(), torch.from_numpy(want["scores"][:n]))
    assert torch.equal(p.labels.cpu(), torch.from_numpy(want["labels"][:n]).to(torch.int64))


@pytest.mark.parametrize("precision", ["fp32", "fp16x3"])
@pytest.mark.parametrize("overview,tile_batch,margin", [(False, 5, 0.0), (True, 4, 0.0), (True, 4, 2.0)],
                         ids=["8 crops in 5 + 3 (one blank), margin 0", "8 crops + overview in 4 + 4 + 1, margin 0",
                              "8 crops + overview in 4 + 4 + 1, margin 2"])
def test_predict_tiled_equals_the_user_route(precision, overview, tile_batch, margin):
    """The synthetic nano weights decode boxes that span their whole 64 x 64 tile whatever the image shows (measured: every
    row is [0, 0, 64, 64] up to a pixel), so at margin 2 every crop row is cut by an interior side and only the overview's
    rows reach the NMS; at margin 0 the crops' rows do (translated, merged per class across tiles).  No image seed changes
    that; the merge's own semantics are covered on hand-made rows above."""
    img = _smooth_image(96, 160, seed=7)
    m_ref, m = _nano(precision), _nano(precision)
    want = _user_route(m_ref, img, TILE, 0.5, overview, tile_batch, margin)
    stats = {}
    got = m.predict_tiled(img, tile=TILE, overlap=0.5, overview=overview, tile_batch=tile_batch, edge_margin=margin, stats=stats)
    print(f"{precision} overview {overview}: per-tile rows {want['per_tile'].tolist()}, merged {want['count']}, border drops "
          f"{want['dropped']}, cross-tile suppressions {want['cross_tile']}; stats {stats}")
    assert want["count"] >= 10
    if margin == 0:
        assert len(set((want["src"][:want["count"]] // m._h.max_out).tolist())) >= 4     # rows of several tiles survive the merge
    assert stats["crops"] == 8 and stats["tiles"] == 8 + int(overview) and stats["trips"] == 0 and stats["d2h_copies"] == 1
    _assert_sample_equals(got, want)
    p = got.pred_instances
    assert torch.equal(p.tiles, torch.from_numpy(want["src"][:want["count"]] // m._h.max_out).to(torch.int64))
    # BGR input: the same image, the same rows
    again = m.predict_tiled(np.ascontiguousarray(img[:, :, ::-1]), tile=TILE, overlap=0.5, overview=overview, tile_batch=tile_batch,
                            edge_margin=margin, channel_order="bgr")
    _assert_sample_equals(again, want)


def test_predict_tiled_of_an_image_that_fits_one_tile_equals_predict():
    from wedetect_amd.detector import DetDataSample
    img = _smooth_image(40, 50, seed=3)
    m_ref, m = _nano("fp16x3"), _nano("fp16x3")
    canvas, meta = _pipeline_canvas(img, TILE)
    ref = m_ref.predict([canvas.permute(2, 0, 1).contiguous()], [DetDataSample(metainfo=meta)])[0].pred_instances
    got = m.predict_tiled(img, tile=TILE).pred_instances
    assert len(ref.scores) >= 1
    for key in ("bboxes", "scores", "labels"):
        assert torch.equal(getattr(ref, key).cpu(), getattr(got, key).cpu()), key


def test_predict_tiled_range_guard_trip_equals_the_in_line_result():
    """tests/test_gpu_feed.py's hot checkpoint: the pipelined steps only detect the trip; the image then runs step by step in
    line through ``checked_counts`` and gives what the in-line route gives, tower state included."""
    import warnings
    from tests.test_gpu_feed import _hot_state
    img = _smooth_image(96, 160, seed=7)
    hot = _hot_state()
    m_ref, m = _nano("fp16x3", hot, calibrate=False), _nano("fp16x3", hot, calibrate=False)
    with warnings.catch_warnings(record=True):
        warnings.simplefilter("always")
        want = _user_route(m_ref, img, TILE, 0.5, True, 4, 0.0)
        stats = {}
        got = m.predict_tiled(img, tile=TILE, overlap=0.5, overview=True, tile_batch=4, edge_margin=0.0, stats=stats)
    t_a, t_b = m_ref._h.tower(4, 64, 64), m._h.tower(4, 64, 64)
    print(f"trip: stats {stats}; in-line trips {t_a.fp16x3_trips} precision {t_a.precision}; tiled trips {t_b.fp16x3_trips} "
          f"precision {t_b.precision}; merged {want['count']}")
    assert stats["trips"] == 1 and stats["inline"] and t_a.fp16x3_trips >= 1
    assert t_b.fp16x3_trips == t_a.fp16x3_trips and t_b.precision == t_a.precision and t_b.overflowed == t_a.overflowed
    assert want["count"] >= 1
    _assert_sample_equals(got, want)
    # while the tower is in its fallback every step goes in line, as the in-line route does
    want2 = _user_route(m_ref, img, TILE, 0.5, True, 4, 0.0)
    stats = {}
    got2 = m.predict_tiled(img, tile=TILE, overlap=0.5, overview=True, tile_batch=4, edge_margin=0.0, stats=stats)
    assert stats["inline"] and stats["trips"] == 0
    _assert_sample_equals(got2, want2)
