"""``YOLOWorldDetector.track`` end to end (GPU): a seeded ``tiny`` detector at 128 x 128 — every field ``predict`` fills unchanged
bit for bit, a static video keeps one id per row across frames and across calls, ``reset_tracks`` starts over, the ids equal
tests/track_ref.py fed with the device's own rows and embeddings (under the margin condition, asserted), the single-label,
top-names and sparse-score steps and per-image banks, cameras (``n_seq = B``), and the happens-before checker on a recorded step."""
import functools

import numpy as np
import pytest
import torch

import tests.track_hazards  # noqa: F401
from tests import hazards as H
from tests import track_ref as R
from tests.test_gpu_tile import NAMES, _smooth_image

pytestmark = pytest.mark.gpu

HW, B, SEED = 128, 4, 20
# the seeded model's scores lie between 0.24 and 0.66 (100 rows kept): a third of the rows is above 0.3
PARAMS = dict(high_thr=0.3, low_thr=0.26, new_thr=0.3, max_age=2)


def _detector(**kw):
    from wedetect_amd import weights as W
    from wedetect_amd.detector import YOLOWorldDetector
    m = YOLOWorldDetector("tiny", test_cfg=dict(max_per_img=100), max_classes=len(NAMES), **kw)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in W.make_state_dict("tiny").items()})
    m.cuda().eval()
    m.set_text_embeddings(torch.from_numpy(W.make_text_bank(len(NAMES))).cuda(), [[n] for n in NAMES])
    return m


def _video(n=B, seed=SEED):
    from wedetect_amd.detector import DetDataSample
    x = torch.from_numpy(_smooth_image(HW, HW, seed=seed)).permute(2, 0, 1).contiguous()
    return [x] * n, [DetDataSample(metainfo=dict(ori_shape=(HW, HW))) for _ in range(n)]


def _params():
    from wedetect_amd.track import TrackParams
    return TrackParams(**PARAMS)


@functools.lru_cache(maxsize=None)
def _world():
    """The default detector, the results of ``predict`` and of two ``track`` calls on the static video, and the device's own rows
    of the second call."""
    m = _detector()
    xs, samples = _video()
    pred = [s.pred_instances for s in m.predict(xs, _video()[1])]
    first = [s.pred_instances for s in m.track(xs, _video()[1], track_params=_params())]
    second = [s.pred_instances for s in m.track(xs, _video()[1], track_params=_params())]
    t = m._h.tower(B, HW, HW)
    torch.cuda.synchronize()
    rows = dict(boxes=t.out_boxes.cpu().numpy().copy(), scores=t.out_scores.cpu().numpy().copy(), labels=t.out_labels.cpu().numpy().copy(),
                count=t.out_count.cpu().numpy().copy(), embed=t.out_embed.cpu().numpy().copy())
    return m, pred, first, second, rows


def test_every_field_of_predict_is_unchanged_bit_for_bit():
    m, pred, first, second, _ = _world()
    for p, a, b in zip(pred, first, second):
        assert len(p.scores) == 100
        for q in (a, b):
            assert torch.equal(p.bboxes.view(torch.int32), q.bboxes.view(torch.int32)) and torch.equal(p.labels, q.labels)
            assert torch.equal(p.scores.view(torch.int32), q.scores.view(torch.int32))
            assert q.track_ids.dtype == torch.int32 and q.track_ids.is_cuda and q.track_ids.shape == q.scores.shape == q.track_hits.shape


def test_a_static_video_keeps_one_id_per_row_across_frames_and_calls_and_reset_starts_over():
    m, pred, first, second, _ = _world()
    s = pred[0].scores.cpu().numpy()
    hi = s >= np.float32(PARAMS["high_thr"])
    assert 10 <= int(hi.sum()) < 100
    ids0 = first[0].track_ids.cpu().numpy()
    assert bool((ids0[hi] > 0).all()) and len(set(ids0[hi].tolist())) == int(hi.sum())     # new_thr == high_thr: every such row is born
    assert sorted(ids0[hi].tolist()) == list(range(1, int(hi.sum()) + 1))                  # in row order, from 1
    assert not ids0[s < np.float32(PARAMS["low_thr"])].any()
    for f, q in enumerate(first + second):
        ids, hits = q.track_ids.cpu().numpy(), q.track_hits.cpu().numpy()
        assert np.array_equal(ids[hi], ids0[hi]), f
        assert bool((hits[hi] == f + 1).all()), f
    assert m._tracker.tracks()[0]["next_id"] == int(hi.sum()) + 1
    # after reset_tracks the ids restart at 1 (the shared detector is left with fresh tracks: the tests above used cached results)
    m.reset_tracks()
    xs, samples = _video()
    again = [q.pred_instances for q in m.track(xs, samples, track_params=_params())]
    assert np.array_equal(again[0].track_ids.cpu().numpy(), ids0) and bool((again[0].track_hits.cpu().numpy()[hi] == 1).all())
    with pytest.raises(ValueError, match="reset_tracks"):
        m.track(xs, samples, n_seq=2)
    from wedetect_amd.track import Tracker
    own = Tracker(1, 128, 768, _params(), device="cuda")                      # an unindexed device names the current one
    with pytest.raises(ValueError, match="carries its own"):
        m.track(xs, samples, tracker=own, track_params=_params())
    mine = [q.pred_instances for q in m.track(xs, samples, tracker=own)]
    assert np.array_equal(mine[0].track_ids.cpu().numpy(), ids0)
    m.reset_tracks()


def test_ids_equal_the_reference_fed_with_the_device_rows():
    m, pred, first, second, rows = _world()
    ref = R.RefTracker(1, 128, 768, R.Params(**PARAMS))
    want = []
    for call in range(2):
        ids, hits = ref.step(rows["boxes"], rows["scores"], rows["labels"], rows["count"], rows["embed"], B)
        want.append((ids, hits))
    print(f"margin {ref.margin:.3e} (threshold {ref.thr_margin:.3e}, picks {ref.pick_margin:.3e}), needed {R.margin_needed(768):.3e}; "
          f"picks {ref.picks}, exact ties {ref.exact_ties}")
    assert ref.margin >= R.margin_needed(768)
    for (ids, hits), got in zip(want, (first, second)):
        for f, q in enumerate(got):
            n = len(q.scores)
            assert n == rows["count"][f]
            assert np.array_equal(q.track_ids.cpu().numpy(), ids[f, :n]) and np.array_equal(q.track_hits.cpu().numpy(), hits[f, :n])
            assert not ids[f, n:].any()


def test_cameras_are_independent_sequences():
    m = _detector()
    xs, samples = _video()
    a = [q.pred_instances.track_ids.cpu().numpy() for q in m.track(xs, samples, n_seq=B, track_params=_params())]
    b = [q.pred_instances.track_ids.cpu().numpy() for q in m.track(xs, _video()[1], n_seq=B, track_params=_params())]
    for f in range(B):
        assert np.array_equal(a[f], a[0]) and np.array_equal(b[f], a[0]) and a[f].max() > 0               # every camera counts from 1
    tr = m._tracker.tracks()
    assert len(tr) == B and all(t["next_id"] == tr[0]["next_id"] > 1 and bool((t["hits"] == 2).all()) for t in tr)


@pytest.mark.parametrize("mode", [dict(best_class=True, agnostic_nms=True), dict(best_class=True, top_names=3), dict(sparse_scores=True)],
                         ids=["best-class-agnostic", "top-names", "sparse-scores"])
def test_the_other_steps_carry_their_embeddings_too(mode):
    m = _detector(**mode)
    xs, samples = _video()
    pred = [s.pred_instances for s in m.predict(xs, _video()[1])]
    p = _params()
    got = [s.pred_instances for s in m.track(xs, samples, track_params=p)]
    ids0 = got[0].track_ids.cpu().numpy()
    hi = pred[0].scores.cpu().numpy() >= np.float32(p.high_thr)
    assert hi.any() and bool((ids0[hi] > 0).all())
    for f, (a, b) in enumerate(zip(pred, got)):
        assert torch.equal(a.bboxes.view(torch.int32), b.bboxes.view(torch.int32)) and torch.equal(a.labels, b.labels)
        assert torch.equal(a.scores.view(torch.int32), b.scores.view(torch.int32))
        if "top_names" in mode:
            assert torch.equal(a.top_labels, b.top_labels) and torch.equal(a.top_scores.view(torch.int32), b.top_scores.view(torch.int32))
        assert np.array_equal(b.track_ids.cpu().numpy()[hi], ids0[hi]) and bool((b.track_hits.cpu().numpy()[hi] == f + 1).all())


def test_per_image_banks():
    from wedetect_amd import weights as W
    from wedetect_amd.detector import DetDataSample
    bank = torch.from_numpy(W.make_text_bank(len(NAMES)))
    row = {n: bank[i] for i, n in enumerate(NAMES)}
    m = _detector()
    m.text_encoder = lambda names: torch.stack([row[n] for n in names]).cuda()
    xs, _ = _video()
    texts = [[[n] for n in NAMES], [[n] for n in NAMES[:-1]]] * 2                          # two class lists alternate in the batch
    mk = lambda: [DetDataSample(metainfo=dict(ori_shape=(HW, HW), texts=t)) for t in texts]
    pred = [s.pred_instances for s in m.predict(xs, mk())]
    got = [s.pred_instances for s in m.track(xs, mk(), n_seq=2, track_params=_params())]
    for a, b in zip(pred, got):
        assert torch.equal(a.bboxes.view(torch.int32), b.bboxes.view(torch.int32)) and torch.equal(a.scores.view(torch.int32), b.scores.view(torch.int32))
    assert got[0].track_ids.max() > 0 and got[2].track_ids.max() > 0


def test_a_recorded_track_step_passes_the_happens_before_checker():
    from tests.test_gpu_hazards import _names, _streams
    m = _detector()
    xs, samples = _video()
    m.track(xs, samples, track_params=_params())                               # warm: weights split, buffers and the tracker exist
    torch.cuda.synchronize()
    t, trk = m._h.tower(B, HW, HW), m._tracker
    names = lambda: {**_names(t)(), "track_state": trk.state, "track_ws": trk._ws, "track_ids": trk._out[(B, 100)][0],
                     "track_hits": trk._out[(B, 100)][1]}
    with H.track(names, _streams(t)) as tr:
        for _ in range(2):
            out = m.track(xs, _video()[1], track_params=_params())
        trk.tracks(with_embed=True)
    assert tr.calls.get("track.track_step", 0) == 2 and tr.calls.get("track.track_export", 0) == 1
    assert len(tr.model.launches) >= 100 and len({s for _, s, _, _ in tr.model.launches}) >= 2
    hz = tr.hazards()
    assert hz == [], H.format_hazards(hz)
    assert int(out[-1].pred_instances.track_hits.max()) == 3 * B                # warm call + two recorded ones, B frames each
    # audit: what the three launches really change is what tests/track_hazards.py declares
    with H.track(names, _streams(t), audit=True) as au:
        m.track(xs, _video()[1], track_params=_params())
        trk.tracks(with_embed=True)
        trk.reset([0])
    assert au.calls.get("track.track_step", 0) == 1 and au.calls.get("track.track_reset", 0) == 1
    assert [x for x in au.mismatches if x[0].startswith("track.")] == [], au.mismatches
