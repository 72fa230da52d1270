"""The guarded-step protocol's host pieces without a device (wedetect_amd/guarded.py): the packed-blob layout, the trip
predicate, and the keyword dicts the tower steps of ``predict`` / ``predict_tiled`` / ``predict_views`` / the streamed mmdet
backend are issued with."""
import types

import numpy as np
import pytest
import torch

from wedetect_amd import guarded as GD
from wedetect_amd.detector import YOLOWorldDetector, _tiled_ctl_parts, _views_ctl_parts
from wedetect_amd.tiling import TILE_DTYPE

F32, I32, U8 = torch.float32, torch.int32, torch.uint8


def _check(parts):
    """Offsets are multiples of 256, parts keep their order and do not overlap, nbytes = last offset + its rounded size."""
    nbytes, lay = GD.layout(parts)
    assert [(n, tuple(s), d) for n, s, d, _, _ in lay] == [(n, tuple(s), d) for n, s, d in parts]
    end = 0
    for name, shape, dt, off, nb in lay:
        assert off % 256 == 0 and off >= end, name
        assert nb == int(np.prod(shape, dtype=np.int64)) * dt.itemsize
        end = off + nb
    last = lay[-1]
    assert nbytes == last[3] + (last[4] + 255) // 256 * 256 and nbytes % 256 == 0
    return nbytes, lay


@pytest.mark.parametrize("total", [1, 7, 8, 9, 33])
def test_layout_of_the_tiled_blobs(total):
    _, lay = _check(_tiled_ctl_parts(total))
    assert [p[0] for p in lay] == ["plan", "meta"] and lay[0][3] == 0 and lay[0][4] == total * TILE_DTYPE.itemsize
    assert lay[1][3] == (total * TILE_DTYPE.itemsize + 255) // 256 * 256 and lay[1][1:3] == ((total, 8), F32)
    max_out, n_steps = 300, -(-total // 4)
    _, lay = _check(GD.merged_parts(max_out, n_steps))
    assert [(n, s, d) for n, s, d, _, _ in lay] == [("out_boxes", (max_out, 4), F32), ("out_scores", (max_out,), F32),
                                                    ("out_labels", (max_out,), I32), ("out_src", (max_out,), I32),
                                                    ("out_count", (1,), I32), ("flags", (n_steps, 2), I32)]
    assert [off for *_, off, _ in lay] == [0, 4864, 6144, 7424, 8704, 8960]       # 4800 -> 4864, 1200 -> 1280, 4 -> 256


@pytest.mark.parametrize("V,B", [(1, 1), (4, 2), (8, 5)])
def test_layout_of_the_views_blobs(V, B):
    _, lay = _check(_views_ctl_parts(V, B))
    assert [(n, s, d) for n, s, d, _, _ in lay] == [("flip", (V,), I32), ("wh", (B, 2), F32), ("meta", (V, B, 8), F32)]
    _, lay = _check(GD.merged_parts(100, V, (B,)))
    assert [(n, s, d) for n, s, d, _, _ in lay] == [("out_boxes", (B, 100, 4), F32), ("out_scores", (B, 100), F32),
                                                    ("out_labels", (B, 100), I32), ("out_src", (B, 100), I32),
                                                    ("out_count", (B,), I32), ("flags", (V, 2), I32)]


def test_layout_is_disjoint_and_aligned_for_random_parts():
    g = np.random.default_rng(11)
    dts = [U8, torch.int16, I32, F32, torch.int64, np.dtype(np.float64), TILE_DTYPE]
    assert GD.layout([]) == (0, [])
    for _ in range(40):
        parts = [(f"p{i}", tuple(int(v) for v in g.integers(0, 9, int(g.integers(0, 4)))), dts[int(g.integers(len(dts)))])
                 for i in range(int(g.integers(1, 9)))]
        nbytes, lay = _check(parts)
        used = set()
        for _, _, _, off, nb in lay:                       # brute force: no byte belongs to two parts, none lies outside
            mine = set(range(off, off + nb))
            assert not (mine & used) and (not mine or max(mine) < nbytes)
            used |= mine
        assert len(used) == sum(nb for *_, nb in lay)


def test_typed_views_share_the_blob():
    nbytes, lay = GD.layout(_views_ctl_parts(3, 2))
    blob = torch.zeros(nbytes, dtype=U8)
    v = GD.typed_views(blob, lay)
    assert {k: (tuple(t.shape), t.dtype) for k, t in v.items()} == {"flip": ((3,), I32), "wh": ((2, 2), F32), "meta": ((3, 2, 8), F32)}
    v["wh"][1, 1] = 1.0
    off = lay[1][3] + 3 * 4
    assert blob[off:off + 4].view(F32).item() == 1.0 and int(blob.count_nonzero()) == 2          # 0x3f800000


def test_trip_predicate():
    x3, f32 = types.SimpleNamespace(precision="fp16x3"), types.SimpleNamespace(precision="fp32")
    assert GD.tripped([3, 0, 7], [[0, 0], [0, 0]], [x3, x3]) is False
    assert GD.tripped([3, -1, 7], [[0, 0], [0, 0]], [x3, x3]) is True
    assert GD.tripped([-1]) is True and GD.tripped([0]) is False
    assert GD.tripped([3, 0], [[0, 0], [0, 1]], [x3, x3]) is True
    assert GD.tripped([3, 0], [[1, 0], [0, 0]], [x3, f32]) is True
    assert GD.tripped([3, 0], [[0, 0], [0, 1]], [x3, f32]) is False       # the same flag, its tower in the fp32 fallback
    assert GD.tripped([3, 0], [[1, 1], [1, 1]], [f32, f32]) is False
    assert GD.tripped([], [[0, 0]], [x3]) is False and GD.tripped([]) is False
    assert GD.tripped([], [[1, 0]], [x3]) is True


BASE = dict(normalize_text=True, score_thr=0.001, iou_thr=0.7, with_embed=False, nms="mmcv", nms_param=10000)
MODES = [
    (dict(), {}, {}),
    (dict(best_class=True), dict(best_class=True, agnostic_nms=False), dict(best_class=True, agnostic_nms=False)),
    (dict(best_class=True, agnostic_nms=True), dict(best_class=True, agnostic_nms=True), dict(best_class=True, agnostic_nms=True)),
    (dict(best_class=True, top_names=5), dict(best_class=True, agnostic_nms=False),
     dict(best_class=True, agnostic_nms=False, top_names=5)),
    (dict(sparse_scores=True, sparse_cap=4096), {}, dict(sparse_scores=True, sparse_cap=4096)),
    (dict(prompt_groups=True), {}, {}),                   # the plan of a bank: ``predict`` adds it for the bank of the batch
]


@pytest.mark.parametrize("ctor,stream_extra,predict_extra", MODES)
def test_step_keywords_of_the_callers(ctor, stream_extra, predict_extra):
    from wedetect_amd.stream import MmdetBackend
    d = YOLOWorldDetector("nano", **ctor)
    assert d._step_kw() == BASE                                                      # predict_tiled, predict_views
    assert MmdetBackend.step_kw(types.SimpleNamespace(det=d)) == dict(BASE, **stream_extra)
    assert d._step_kw(modes=True) == dict(BASE, **predict_extra)                     # predict
    d = YOLOWorldDetector("nano", test_cfg=dict(score_thr=0.05, nms=dict(type="nms", iou_threshold=0.5, split_thr=2000)), **ctor)
    base = dict(normalize_text=True, score_thr=0.05, iou_thr=0.5, with_embed=False, nms="mmcv", nms_param=2000)
    assert d._step_kw() == base and d._step_kw(modes=True) == dict(base, **predict_extra)
    assert MmdetBackend.step_kw(types.SimpleNamespace(det=d)) == dict(base, **stream_extra)
