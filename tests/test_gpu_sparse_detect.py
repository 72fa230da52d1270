"""ImageTower.detect(sparse_scores=True) (GPU): the sparse step against the dense multi-label step of the SAME tower with the
text fold off (WEDETECT_FOLD_TEXT=0: the unfolded head both run on), tensor for tensor — K = 300 on an fp16x3 tower takes the
fused kernel, K = 80 wd_sparse_rows — in line and pipelined, the overflow fallback of checked_counts(), an fp32 tower, per-image
banks, the detector's keyword and the entry script's flag.  Tiny tower, 2 x 160 x 160: 525 anchors per image, random weights.
Every threshold is chosen from the dense step's own scores so that no list overflows."""
import json
import os
import warnings

import numpy as np
import pytest
import torch

import tests.sparse_hazards  # noqa: F401
from tests.test_gpu_best_detect import _meta
from tests.test_gpu_hazards import _bank, _batches, _configure
from tests.test_gpu_network import build

pytestmark = pytest.mark.gpu

B, HW, IOU = 2, 160, 0.7
FIELDS = ("bboxes", "scores", "labels", "anchors", "count", "embeddings")


def _tower(precision="fp16x3"):
    _, t, imgs = build("tiny", B, HW, num_prompts=48, precision=precision, max_classes=80)
    t.fold_text = False                                          # what WEDETECT_FOLD_TEXT=0 sets: the dense step on the unfolded head
    return t, torch.from_numpy(imgs).cuda()


def _threshold(t, batches, text, want=3000, counts=None):
    """A threshold from the dense scores of these batches: about ``want`` candidates per image, asserted below the list capacity."""
    per = []
    for x in batches:
        t.features(x, num_classes=None if text.dim() == 3 else text.shape[0])
        s = t.similarity(text, normalize=True, text_counts=counts)
        torch.cuda.synchronize()
        per.append(s.reshape(B, -1).cpu().numpy().copy())
    flat = np.sort(np.concatenate([p.reshape(-1) for p in per]))
    thr = float(flat[-want * B * len(batches)])
    seen = [int((p[b] > np.float32(thr)).sum()) for p in per for b in range(B)]
    assert 0 < min(seen) and max(seen) <= 30000, seen
    return thr, seen


def _snap(r):
    torch.cuda.synchronize()
    return {n: v.clone() for n, v in r.items()}


@pytest.mark.parametrize("k", [300, 80])
def test_sparse_step_equals_the_dense_step_in_line_and_pipelined(k):
    from wedetect_amd import sparse as SP
    t, _ = _tower()
    meta, batches, text = _meta(t), _batches(B, HW, n=3), _bank(k)
    thr, seen = _threshold(t, batches, text)
    kw = dict(normalize_text=True, score_thr=thr, iou_thr=IOU, with_embed=True, nms="mmcv")
    dense = [_snap(t.detect(x, text, meta, **kw)) for x in batches]
    shape0 = tuple(t.scores.shape)
    calls = {}
    real_f, real_r = SP.sparse_similarity_split, SP.sparse_rows
    SP.sparse_similarity_split = lambda *a, **kw_: (calls.__setitem__("fused", calls.get("fused", 0) + 1), real_f(*a, **kw_))[1]
    SP.sparse_rows = lambda *a, **kw_: (calls.__setitem__("rows", calls.get("rows", 0) + 1), real_r(*a, **kw_))[1]
    try:
        inline = [_snap(t.detect(x, text, meta, sparse_scores=True, **kw)) for x in batches]
        _configure(t, depth="2")
        piped = []
        for x in batches:                                        # back to back, no host synchronisation in between
            r = t.detect(x, text, meta, overlap_post=True, sparse_scores=True, **kw)
            with torch.cuda.stream(t.post_stream):
                piped.append({n: v.clone() for n, v in r.items()})
        t.wait_post()
        torch.cuda.synchronize()
    finally:
        SP.sparse_similarity_split, SP.sparse_rows = real_f, real_r
    assert calls == ({"fused": 6} if k >= t.SIM_SPLIT_MIN else {"rows": 6}), calls
    assert tuple(t.scores.shape) == shape0 and int(t.range_flags.max()) == 0
    assert tuple(t._sparse_list.shape) == (B, 65536)
    for i, d in enumerate(dense):
        for got in (inline[i], piped[i]):
            for n in FIELDS:
                assert torch.equal(got[n], d[n]), f"batch {i}: {n}"
            assert got["sparse_status"].tolist() == [0, 0] and got["sparse_seen"].tolist() == seen[B * i:B * i + B]
        assert int(d["count"].min()) > 0
    assert t.checked_counts(t.detect(batches[0], text, meta, sparse_scores=True, **kw), None) == dense[0]["count"].tolist()
    assert (t.sparse_overflows, t.sparse_declined) == (0, 0)
    with pytest.raises(ValueError, match="best_class"):
        t.detect(batches[0], text, meta, sparse_scores=True, best_class=True, **kw)


def test_overflowing_lists_rerun_densely_and_the_tower_stops_trying():
    t, x = _tower()
    meta, text = _meta(t), _bank(300)
    kw = dict(normalize_text=True, score_thr=0.0, iou_thr=IOU, with_embed=True, nms="mmcv")
    dense = _snap(t.detect(x, text, meta, **kw))
    run = lambda: t.detect(x, text, meta, sparse_scores=True, sparse_cap=1024, **kw)
    seen = []
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        for step in range(4):
            res = run()
            if step < 2:
                torch.cuda.synchronize()
                assert res["sparse_status"].tolist() == [1, 1] and res["count"].tolist() == [0, 0]
                assert res["sparse_seen"].tolist() == [t.ntot * 300] * 2
            counts = t.checked_counts(res, run)
            torch.cuda.synchronize()
            assert counts == dense["count"].tolist()
            for n in FIELDS:                                     # the tower's buffers hold the dense re-run's result
                assert torch.equal(res[n], dense[n]), f"step {step}: {n}"
            seen.append((t.sparse_overflows, t.sparse_declined))
    assert seen == [(1, 0), (2, 0), (2, 1), (2, 2)], seen
    assert len([m for m in w if "sparse candidate lists overflowed" in str(m.message)]) == 1
    # another threshold starts afresh: sparse again, complete lists
    thr, _ = _threshold(t, [x], text)
    res = _snap(t.detect(x, text, meta, sparse_scores=True, sparse_cap=1024, **{**kw, "score_thr": thr}))
    assert res["sparse_status"].tolist() == [0, 0] and t.sparse_declined == 2


def _hot_embed(t, factor=3e5):
    """The three embedding convs scaled by ``factor``: the region embeddings leave the fp16 range, so the fp16x3 similarity launch
    meets inf halves (non-finite accumulators: the range flag and status 2) while the fp32 kernels score the same rows finitely."""
    for l in range(3):
        t.P[f"head{l}.embed.w"].mul_(factor)
        t.P[f"head{l}.embed.b"].mul_(factor)


def test_overflow_that_shows_only_in_the_fp32_rerun_of_a_range_trip_is_rerun_densely():
    """Status 2 hides status 1: the first (fp16x3) step reports every image non-finite, the range guard switches the tower to the
    fp32 kernels and re-runs the step — sparse again, through wd_sparse_rows — and only that re-run can show that the lists
    overflow (score_thr 0, 32768 keys for 157 500 pairs).  Its status is read too: the step is run once more densely and the
    result is the dense fp32 step's, tensor for tensor."""
    ref, x = _tower("fp32")
    _hot_embed(ref)
    meta, text = _meta(ref), _bank(300)
    kw = dict(normalize_text=True, score_thr=0.0, iou_thr=IOU, with_embed=True, nms="mmcv")
    want = _snap(ref.detect(x, text, meta, **kw))
    assert int(want["count"].min()) > 0 and bool(torch.isfinite(want["scores"]).all())
    t, _ = _tower()
    _hot_embed(t)
    run = lambda: t.detect(x, text, meta, sparse_scores=True, sparse_cap=1024, **kw)
    res = run()
    torch.cuda.synchronize()
    assert res["sparse_status"].tolist() == [2, 2] and res["count"].tolist() == [-1, -1] and int(t.range_flags.max()) == 1
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        counts = t.checked_counts(res, run)
    torch.cuda.synchronize()
    assert t.precision == "fp32" and t.overflowed and t.fp16x3_trips == 1
    assert any("fp16 range" in str(m.message) for m in w)
    assert int(t._sparse_seen.min()) > t._sparse_list.shape[1] == 32768      # the fp32 re-run's lists did overflow
    assert (t.sparse_overflows, t.sparse_declined) == (1, 0)
    assert counts == want["count"].tolist()
    for n in FIELDS:
        assert torch.equal(res[n], want[n]), n
    # the list only grows: a later, larger request replaces it, a smaller one keeps it
    t.detect(x, text, meta, sparse_scores=True, sparse_cap=65536, **{**kw, "score_thr": 2.0})
    t.detect(x, text, meta, sparse_scores=True, sparse_cap=1024, overlap_post=True, **{**kw, "score_thr": 2.0})
    t.wait_post()
    torch.cuda.synchronize()
    assert tuple(t._sparse_list.shape) == (B, 65536)


def test_fp32_tower_and_per_image_banks_give_the_dense_result():
    t, x = _tower("fp32")
    meta, text = _meta(t), _bank(300)
    thr, _ = _threshold(t, [x], text)
    kw = dict(normalize_text=True, score_thr=thr, iou_thr=IOU, with_embed=True, nms="mmcv")
    dense = _snap(t.detect(x, text, meta, **kw))
    got = _snap(t.detect(x, text, meta, sparse_scores=True, **kw))
    for n in FIELDS:
        assert torch.equal(got[n], dense[n]), n
    assert got["sparse_status"].tolist() == [0, 0] and int(dense["count"].min()) > 0
    t, x = _tower()
    meta = _meta(t)
    text = torch.stack([_bank(80, seed=100), _bank(80, seed=200)]).contiguous()
    counts = torch.tensor([7, 80], dtype=torch.int32, device="cuda")
    thr, _ = _threshold(t, [x], text, want=300, counts=counts)
    kw = dict(normalize_text=True, score_thr=thr, iou_thr=IOU, with_embed=True, nms="mmcv", text_counts=counts)
    dense = _snap(t.detect(x, text, meta, **kw))
    for overlap in (False, True):
        r = t.detect(x, text, meta, sparse_scores=True, overlap_post=overlap, **kw)
        t.wait_post()
        got = _snap(r)
        for n in FIELDS:
            assert torch.equal(got[n], dense[n]), (overlap, n)
        assert got["sparse_status"].tolist() == [0, 0]
    n0 = int(dense["count"][0])
    assert n0 > 0 and int(dense["labels"][0, :n0].max()) < 7


def _detector(**kw):
    from wedetect_amd import weights as W
    from wedetect_amd.detector import YOLOWorldDetector
    sd_np = W.make_state_dict("nano")
    model = YOLOWorldDetector("nano", test_cfg=dict(max_per_img=50, score_thr=0.3), max_classes=81, **kw)
    model.load_state_dict({"state_dict": {n: torch.from_numpy(v) for n, v in sd_np.items()}})
    model.cuda().eval()
    model.set_text_embeddings(torch.from_numpy(W.make_text_bank(81) * np.float32(2.5)))
    return model


def test_detector_keyword_gives_the_default_detectors_predictions(monkeypatch):
    from wedetect_amd import weights as W
    from wedetect_amd.detector import DetDataSample
    monkeypatch.setenv("WEDETECT_FOLD_TEXT", "0")
    rgb = W.make_images(2, 128, 128, seed=77)
    bgr_chw = [torch.from_numpy(np.ascontiguousarray(im[..., ::-1].transpose(2, 0, 1))) for im in rgb]
    metas = [dict(ori_shape=(200, 256), scale_factor=(0.5, 0.5), pad_param=np.array([14., 14., 0., 0.])),
             dict(ori_shape=(128, 100), scale_factor=(1.0, 1.0), pad_param=np.array([0., 0., 14., 14.]))]
    out = {}
    for name, kw in (("dense", {}), ("sparse", dict(sparse_scores=True))):
        model = _detector(**kw)
        res = model.test_step(dict(inputs=bgr_chw, data_samples=[DetDataSample(metainfo=m) for m in metas]))
        out[name] = [(r.pred_instances.bboxes.cpu(), r.pred_instances.scores.cpu(), r.pred_instances.labels.cpu()) for r in res]
        if kw:
            assert not model._h._graphs                          # the sparse step is eager
            tower = model._h.tower(2, 128, 128)
            assert tower._sparse_list is not None and (tower.sparse_overflows, tower.sparse_declined) == (0, 0)
    kept = 0
    for d, s in zip(out["dense"], out["sparse"]):
        assert all(torch.equal(a, b) for a, b in zip(d, s))
        kept += len(d[1])
    assert kept > 0


def test_infer_wedetect_flag_writes_the_same_json(tmp_path, monkeypatch):
    """infer_wedetect.main with and without --sparse-scores on one 320 x 320 image (the test pipeline letterboxes it): the dumped
    detections are the same.  --sparse-cap 2^20 holds every pair of 8400 anchors x 81 classes, so no list overflows at the
    config's score_thr."""
    from PIL import Image
    import infer_wedetect as iw
    from tests.test_gpu_entry import ROOT, _text_tower, toy_tokenizer
    from wedetect_amd import weights as W
    monkeypatch.setenv("WEDETECT_FOLD_TEXT", "0")
    vocab = 400
    _, _, text_sd = _text_tower(vocab=vocab)
    sd_np = W.make_state_dict("tiny")
    ckpt_path = str(tmp_path / "wedetect_tiny.pth")
    torch.save({"state_dict": {**{k: torch.from_numpy(v) for k, v in sd_np.items()}, **text_sd}, "meta": {}}, ckpt_path)
    img_path = str(tmp_path / "synthetic.png")
    Image.fromarray(W.make_images(1, 320, 320, seed=1234)[0]).save(img_path)
    (tmp_path / "names.txt").write_text("\n".join(f"class {i}" for i in range(80)) + "\n", encoding="utf-8")
    dumped = {}
    for name, extra in (("dense", []), ("sparse", ["--sparse-scores", "--sparse-cap", str(1 << 20)])):
        out_dir = str(tmp_path / name)
        res = iw.main(["--config", os.path.join(ROOT, "config", "wedetect_tiny.py"), "--checkpoint", ckpt_path, "--image", img_path,
                       "--text", str(tmp_path / "names.txt"), "--threshold", "0.05", "--topk", "100", "--device", "cuda:0",
                       "--output-dir", out_dir, "--dump-json", *extra], tokenizer=toy_tokenizer(vocab))
        assert len(res) == 1
        dumped[name] = json.load(open(os.path.join(out_dir, "synthetic.json")))
    assert dumped["sparse"] == dumped["dense"] and len(dumped["dense"]["scores"]) > 0
