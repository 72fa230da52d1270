"""ImageTower.detect(best_class=True) (GPU): the single-label step against tests/best_ref.py applied to the tower's OWN
materialised similarity() scores and boxes — K = 80 takes the materialised path (similarity launch + wd_best_rows), K = 300 on
an fp16x3 tower the fused kernel — in line and pipelined, shared and per-image banks, a bank of 20 000 rows that is never
materialised, and the detector's keywords.  Tiny tower, 2 x 160 x 160: 525 anchors per image, random weights."""
import numpy as np
import pytest
import torch

import tests.best_hazards  # noqa: F401
from tests import best_ref as R
from tests import hazards as H
from tests.test_gpu_hazards import _bank, _batches, _clean, _configure, _names, _stream_of_batches, _streams
from tests.test_gpu_network import build
from tests.util import assert_close

pytestmark = pytest.mark.gpu

B, HW, THR, IOU = 2, 160, 0.001, 0.7
TOL = 1e-3                                   # tests/util.py compare_kept_lists: score_tol of the detect tests


def _meta(t, pre=1.0):
    """Letterbox metadata of two different images: pad, scale, original size; the mmdet order (rescale before NMS)."""
    m = torch.tensor([[4.0, 2.0, 0.0, 0.5, 0.5, 300.0, 310.0, pre], [0.0, 6.0, 0.0, 1.25, 1.25, 128.0, 118.0, pre]], dtype=torch.float32)
    return m[: t.B].contiguous().to(t.dev)


def _materialised(t, x, text, counts=None):
    """The tower's own similarity() scores and boxes for this batch (host arrays)."""
    t.features(x, num_classes=None if text.dim() == 3 else text.shape[0])
    s = t.similarity(text, normalize=True, text_counts=counts)
    torch.cuda.synchronize()
    return s.cpu().numpy().copy(), t.boxes.cpu().numpy().copy()


def _check(name, res, scores, boxes, meta, t, split_thr, agnostic, counts=None):
    meta = meta.cpu().numpy()
    kept = 0
    for i in range(scores.shape[0]):
        sc = scores[i] if counts is None else scores[i][:, : int(counts[i])]
        o = R.predict_image(boxes[i], sc, meta[i], THR, t.nms_pre, IOU, t.max_out, split_thr, agnostic)
        n = int(res["count"][i])
        assert n == o["scores"].shape[0], f"{name} image {i}: {n} rows, reference {o['scores'].shape[0]}"
        assert np.array_equal(res["anchors"][i, :n].cpu().numpy(), o["anchors"]), f"{name} image {i}: anchors"
        assert np.array_equal(res["labels"][i, :n].cpu().numpy(), o["labels"]), f"{name} image {i}: labels"
        assert_close(f"{name} image {i} scores", res["scores"][i, :n], o["scores"], TOL)
        assert_close(f"{name} image {i} boxes", res["bboxes"][i, :n], o["bboxes"], TOL, 1e-5)
        assert bool((res["labels"][i, n:] == -1).all()) and bool((res["anchors"][i, n:] == -1).all())
        if counts is not None and n:
            assert int(res["labels"][i, :n].max()) < int(counts[i])
        kept += n
    assert kept > 0, f"{name}: nothing was kept — the case checks nothing"
    return kept


@pytest.mark.parametrize("precision", ["fp32", "fp16x3"])
@pytest.mark.parametrize("agnostic", [False, True])
@pytest.mark.parametrize("k", [80, 300])
def test_best_class_step_equals_the_reference_on_the_towers_own_scores(k, agnostic, precision):
    from wedetect_amd import best as BS
    _, t, imgs = build("tiny", B, HW, num_prompts=48, precision=precision, max_classes=80)
    x, meta, text = torch.from_numpy(imgs).cuda(), _meta(t), _bank(k)
    calls = {}
    real_f, real_r = BS.best_similarity_split, BS.best_rows
    BS.best_similarity_split = lambda *a, **kw: (calls.__setitem__("fused", calls.get("fused", 0) + 1), real_f(*a, **kw))[1]
    BS.best_rows = lambda *a, **kw: (calls.__setitem__("rows", calls.get("rows", 0) + 1), real_r(*a, **kw))[1]
    try:
        got = {}
        for split_thr in (10000, 64):                        # one pass across the labels / per label (525 candidates >= 64)
            r = t.detect(x, text, meta, normalize_text=True, score_thr=THR, iou_thr=IOU, with_embed=True, nms="mmcv", nms_param=split_thr,
                         best_class=True, agnostic_nms=agnostic)
            torch.cuda.synchronize()
            got[split_thr] = {n: v.clone() for n, v in r.items()}
    finally:
        BS.best_similarity_split, BS.best_rows = real_f, real_r
    fused = precision == "fp16x3" and k >= t.SIM_SPLIT_MIN
    assert calls == ({"fused": 2} if fused else {"rows": 2}), calls
    assert t.scores.shape[2] == (80 if fused else max(80, k)) and int(t.range_flags.max()) == 0      # fused: the score tensor did not grow
    scores, boxes = _materialised(t, x, text)
    embed = t.embed.cpu().numpy()
    for split_thr, res in got.items():
        _check(f"K {k} split_thr {split_thr}", res, scores, boxes, meta, t, split_thr, agnostic)
        for i in range(B):
            n = int(res["count"][i])
            assert np.array_equal(res["embeddings"][i, :n].cpu().numpy(), embed[i][res["anchors"][i, :n].cpu().numpy()])
    with pytest.raises(NotImplementedError, match="best_class"):
        t.detect(x, text, meta, normalize_text=True, score_thr=THR, nms="mmcv", agnostic_nms=True)
    with pytest.raises(ValueError):
        t.detect(x, text, meta, normalize_text=True, score_thr=THR, nms="torchvision", best_class=True, agnostic_nms=True)


@pytest.mark.parametrize("k,precision", [(80, "fp16x3"), (300, "fp16x3"), (300, "fp32")])
def test_pipelined_best_class_steps_equal_the_in_line_step_and_are_ordered(k, precision):
    """Six different batches back to back with overlap_post=True: tensor for tensor the in-line results, and every conflicting
    pair of launches ordered (tests/hazards.py with the wrappers of wedetect_amd/best.py declared by tests/best_hazards.py)."""
    _, t, _ = build("tiny", B, HW, num_prompts=48, precision=precision, max_classes=80)
    meta, batches, text = _meta(t), _batches(B, HW), _bank(k)
    kw = dict(normalize_text=True, score_thr=THR, iou_thr=IOU, with_embed=True, nms="mmcv", best_class=True, agnostic_nms=True)
    _configure(t, depth="2")
    inline = []
    for x in batches:
        r = t.detect(x, text, meta, **kw)
        torch.cuda.synchronize()
        inline.append({n: v.clone() for n, v in r.items()})
    names = lambda: {**_names(t)(), "best_key": t._best_key, "best_score": t._best_score, "best_label": t._best_label}
    with H.track(names, _streams(t)) as tr:
        got, last = _stream_of_batches(t, batches, [text], meta, **kw)
    assert t.post_stream is not None and t._nh_stream is not None
    for i, (g, w) in enumerate(zip(got, inline)):
        for n in w:
            assert torch.equal(g[n], w[n]), f"step {i}: {n}"
        assert int(g["count"].min()) > 0 and not bool(g["range_flags"].any())
    for n in inline[0]:
        assert torch.equal(last[n], inline[0][n])
    want = "best.best_similarity_split" if (precision == "fp16x3" and k >= 256) else "best.best_rows"
    assert tr.calls.get(want, 0) == 7 and tr.calls.get("best.best_unpack", 0) == 7 and tr.calls.get("best.nms_gather_labeled", 0) == 7
    assert "lib.nms_gather" not in tr.calls and "fold.fold_similarity" not in tr.calls
    _clean(tr)


def test_per_image_banks_keep_their_labels_below_their_counts():
    _, t, imgs = build("tiny", B, HW, num_prompts=48, precision="fp16x3", max_classes=80)
    x, meta = torch.from_numpy(imgs).cuda(), _meta(t)
    text = torch.stack([_bank(80, seed=100), _bank(80, seed=200)]).contiguous()
    counts = torch.tensor([7, 80], dtype=torch.int32, device="cuda")
    kw = dict(normalize_text=True, score_thr=THR, iou_thr=IOU, with_embed=False, nms="mmcv", text_counts=counts, best_class=True)
    r = t.detect(x, text, meta, **kw)
    torch.cuda.synchronize()
    res = {n: v.clone() for n, v in r.items()}
    scores, boxes = _materialised(t, x, text, counts)
    _check("per-image banks", res, scores, boxes, meta, t, 10000, False, counts=counts.tolist())
    r2 = t.detect(x, text, meta, overlap_post=True, **kw)
    t.wait_post()
    torch.cuda.synchronize()
    for n in res:
        assert torch.equal(r2[n], res[n]), n


def test_a_bank_of_20000_rows_is_never_materialised():
    """B = 1, K = 20 000 on the fused path: ``tower.scores`` keeps its size and the step's peak allocation stays within
    rows * K * 4 bytes (42 MB: the score tensor) of the K = 300 step's.  Both banks have been seen once before the measured
    steps: their split copies belong to the bank, not to the step, and exist in the multi-label step too."""
    _, t, imgs = build("tiny", 1, HW, num_prompts=48, precision="fp16x3", max_classes=80)
    x, meta = torch.from_numpy(imgs).cuda(), _meta(t)
    small, big = _bank(300), _bank(20000)
    kw = dict(normalize_text=True, score_thr=THR, iou_thr=IOU, with_embed=False, nms="mmcv", best_class=True, agnostic_nms=True)
    peaks = {}
    for name, bank in (("small", small), ("big", big)):
        t.detect(x, bank, meta, **kw)
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        r = t.detect(x, bank, meta, **kw)
        torch.cuda.synchronize()
        peaks[name] = torch.cuda.max_memory_allocated() - base
        assert int(r["count"][0]) > 0 and int(t.range_flags.max()) == 0
        labels = r["labels"][0, : int(r["count"][0])]
        assert int(labels.min()) >= 0 and int(labels.max()) < bank.shape[0]
    rows = t.ntot
    print(f"peak allocation above the step's start: K 300 {peaks['small']} B, K 20000 {peaks['big']} B; score tensor would be {rows * 20000 * 4} B")
    assert tuple(t.scores.shape) == (1, rows, 80)
    assert peaks["big"] - peaks["small"] < rows * 20000 * 4
    assert int(r["labels"][0, : int(r["count"][0])].max()) >= 300           # names beyond the small bank are found


def test_detector_keywords_give_one_label_per_box_and_tiled_inference_refuses():
    from wedetect_amd import weights as W
    from wedetect_amd.detector import DetDataSample, YOLOWorldDetector
    sd_np = W.make_state_dict("nano")
    model = YOLOWorldDetector("nano", test_cfg=dict(max_per_img=50), max_classes=81, best_class=True, agnostic_nms=True)
    model.load_state_dict({"state_dict": {n: torch.from_numpy(v) for n, v in sd_np.items()}})
    model.cuda().eval()
    model.set_text_embeddings(torch.from_numpy(W.make_text_bank(81) * np.float32(2.5)))
    rgb = W.make_images(2, 128, 128, seed=77)
    bgr_chw = [torch.from_numpy(np.ascontiguousarray(im[..., ::-1].transpose(2, 0, 1))) for im in rgb]
    metas = [dict(ori_shape=(200, 256), scale_factor=(0.5, 0.5), pad_param=np.array([14., 14., 0., 0.])),
             dict(ori_shape=(128, 100), scale_factor=(1.0, 1.0), pad_param=np.array([0., 0., 14., 14.]))]
    res = model.test_step(dict(inputs=bgr_chw, data_samples=[DetDataSample(metainfo=m) for m in metas]))
    assert len(res) == 2
    for r in res:
        pi = r.pred_instances
        n = len(pi.scores)
        assert 0 < n <= 50 and tuple(pi.bboxes.shape) == (n, 4) and tuple(pi.labels.shape) == (n,)
        assert int(pi.labels.min()) >= 0 and int(pi.labels.max()) < 81
        assert bool((pi.scores[:-1] >= pi.scores[1:]).all())
    assert not model._h._graphs                              # the single-label step is eager
    with pytest.raises(NotImplementedError, match="best_class"):
        model.predict_tiled(np.zeros((300, 300, 3), np.uint8))
