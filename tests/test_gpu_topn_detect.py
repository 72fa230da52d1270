"""ImageTower.detect(best_class=True, top_names=n) (GPU): every field of the best-class step unchanged bit for bit, the name lists
against tests/topn_ref.py applied to the tower's OWN materialised similarity() scores — K = 80 and per-image banks take the block
path (similarity launch + wd_topn_rows), K = 300 on an fp16x3 tower the fused kernel — in line and pipelined, under the
happens-before checker, and the detector's keyword.  Tiny tower, 2 x 160 x 160: 525 anchors per image, random weights."""
import numpy as np
import pytest
import torch

import tests.best_hazards  # noqa: F401
import tests.topn_hazards  # noqa: F401
from tests import hazards as H
from tests import topn_ref as R
from tests.test_gpu_best_detect import B, HW, IOU, THR, _materialised, _meta
from tests.test_gpu_hazards import _bank, _batches, _clean, _configure, _names, _stream_of_batches, _streams
from tests.test_gpu_network import build

pytestmark = pytest.mark.gpu

N_TOP = 5


def _clone(r):
    return {n: v.clone() for n, v in r.items()}


def _check_lists(name, res, base, scores, n_top, counts=None):
    """``res`` (top_names step) against ``base`` (best-class step) and the dense ``scores`` [B, N, K] of similarity()."""
    for f in base:
        assert torch.equal(res[f], base[f]), f"{name}: field {f} differs from the best-class step"
    ts, tl = res["top_scores"], res["top_labels"]
    assert tuple(ts.shape) == tuple(tl.shape) == (scores.shape[0], res["scores"].shape[1], n_top) and ts.dtype == torch.float32 and tl.dtype == torch.int32
    kept = 0
    for i in range(scores.shape[0]):
        n = int(res["count"][i])
        kept += n
        k_i = scores.shape[2] if counts is None else int(counts[i])
        assert torch.equal(tl[i, :n, 0], res["labels"][i, :n]) and torch.equal(ts[i, :n, 0].view(torch.int32), res["scores"][i, :n].view(torch.int32))
        anc = res["anchors"][i, :n].cpu().numpy()
        ws, wl = R.top_n(scores[i][anc][:, :k_i], n_top)
        assert np.array_equal(ts[i, :n].cpu().numpy().view(np.uint32), ws.view(np.uint32)), f"{name} image {i}: list scores"
        assert np.array_equal(tl[i, :n].cpu().numpy(), wl), f"{name} image {i}: list labels"
        assert not bool(ts[i, n:].any()) and bool((tl[i, n:] == -1).all())          # rows past the count: (0, -1)
    assert kept > 0, f"{name}: nothing was kept — the case checks nothing"


@pytest.mark.parametrize("precision", ["fp32", "fp16x3"])
@pytest.mark.parametrize("agnostic", [False, True])
@pytest.mark.parametrize("k", [80, 300])
def test_top_names_step_keeps_every_best_class_field_and_lists_the_reference_names(k, agnostic, precision):
    from wedetect_amd import topn as TN
    _, t, imgs = build("tiny", B, HW, num_prompts=48, precision=precision, max_classes=80)
    x, meta, text = torch.from_numpy(imgs).cuda(), _meta(t), _bank(k)
    kw = dict(normalize_text=True, score_thr=THR, iou_thr=IOU, with_embed=True, nms="mmcv", best_class=True, agnostic_nms=agnostic)
    base = _clone(t.detect(x, text, meta, **kw))
    torch.cuda.synchronize()
    gen, shape = t.generation, tuple(t.scores.shape)
    calls = {}
    real_f, real_r = TN.topn_similarity_split, TN.topn_rows
    TN.topn_similarity_split = lambda *a, **kw_: (calls.__setitem__("fused", calls.get("fused", 0) + 1), real_f(*a, **kw_))[1]
    TN.topn_rows = lambda *a, **kw_: (calls.__setitem__("rows", calls.get("rows", 0) + 1), real_r(*a, **kw_))[1]
    try:
        res = _clone(t.detect(x, text, meta, top_names=N_TOP, **kw))
        torch.cuda.synchronize()
        res8 = _clone(t.detect(x, text, meta, top_names=8, **kw))
        torch.cuda.synchronize()
    finally:
        TN.topn_similarity_split, TN.topn_rows = real_f, real_r
    fused = precision == "fp16x3" and k >= t.SIM_SPLIT_MIN
    assert calls == ({"fused": 2} if fused else {"rows": 2}), calls
    assert int(t.range_flags.max()) == 0
    # a call without the keyword after calls with it: what it returned before, nothing re-allocated
    again = _clone(t.detect(x, text, meta, **kw))
    torch.cuda.synchronize()
    assert set(again) == set(base) and all(torch.equal(again[f], base[f]) for f in base)
    assert t.generation == gen and tuple(t.scores.shape) == shape
    scores, _ = _materialised(t, x, text)
    _check_lists(f"K {k} n {N_TOP}", res, base, scores, N_TOP)
    _check_lists(f"K {k} n 8", res8, base, scores, 8)
    assert torch.equal(res8["top_labels"][:, :, :N_TOP], res["top_labels"]) and torch.equal(res8["top_scores"][:, :, :N_TOP], res["top_scores"])
    with pytest.raises(ValueError, match="best_class"):
        t.detect(x, text, meta, normalize_text=True, score_thr=THR, nms="mmcv", top_names=3)
    with pytest.raises(ValueError, match="0..8"):
        t.detect(x, text, meta, top_names=9, **kw)


def test_per_image_banks_with_ragged_counts_take_the_block_path():
    _, t, imgs = build("tiny", B, HW, num_prompts=48, precision="fp16x3", max_classes=80)
    x, meta = torch.from_numpy(imgs).cuda(), _meta(t)
    text = torch.stack([_bank(80, seed=100), _bank(80, seed=200)]).contiguous()
    counts = torch.tensor([3, 80], dtype=torch.int32, device="cuda")             # image 0: fewer names than slots
    kw = dict(normalize_text=True, score_thr=THR, iou_thr=IOU, with_embed=False, nms="mmcv", text_counts=counts, best_class=True)
    base = _clone(t.detect(x, text, meta, **kw))
    res = _clone(t.detect(x, text, meta, top_names=N_TOP, **kw))
    torch.cuda.synchronize()
    scores, _ = _materialised(t, x, text, counts)
    _check_lists("per-image banks", res, base, scores, N_TOP, counts=counts.tolist())
    n0 = int(res["count"][0])
    assert n0 > 0 and bool((res["top_labels"][0, :n0, 3:] == -1).all()) and bool((res["top_labels"][0, :n0, :3] >= 0).all())
    r2 = t.detect(x, text, meta, overlap_post=True, top_names=N_TOP, **kw)
    t.wait_post()
    torch.cuda.synchronize()
    for n in res:
        assert torch.equal(r2[n], res[n]), n


@pytest.mark.parametrize("k,precision,agnostic", [(80, "fp16x3", False), (300, "fp16x3", True), (300, "fp16x3", False), (300, "fp32", True),
                                                  (80, "fp32", False)])
def test_pipelined_top_names_steps_equal_the_in_line_steps_and_are_ordered(k, precision, agnostic):
    """Six different batches back to back with overlap_post=True: tensor for tensor the in-line results (those of the best-class
    step among them), and every conflicting pair of launches ordered — the keys are cleared by step i + 1 behind wait_post()."""
    _, t, _ = build("tiny", B, HW, num_prompts=48, precision=precision, max_classes=80)
    meta, batches, text = _meta(t), _batches(B, HW), _bank(k)
    kw = dict(normalize_text=True, score_thr=THR, iou_thr=IOU, with_embed=True, nms="mmcv", best_class=True, agnostic_nms=agnostic)
    _configure(t, depth="2")
    inline, best = [], []
    for x in batches:
        best.append(_clone(t.detect(x, text, meta, **kw)))
        torch.cuda.synchronize()
        inline.append(_clone(t.detect(x, text, meta, top_names=N_TOP, **kw)))
        torch.cuda.synchronize()
    names = lambda: {**_names(t)(), "best_key": t._best_key, "best_score": t._best_score, "best_label": t._best_label,
                     "topn_key": t._topn_key, "topn_out_score": t._topn_out_score, "topn_out_label": t._topn_out_label}
    with H.track(names, _streams(t)) as tr:
        got, last = _stream_of_batches(t, batches, [text], meta, top_names=N_TOP, **kw)
    assert t.post_stream is not None and t._nh_stream is not None
    for i, (g, w, bst) in enumerate(zip(got, inline, best)):
        for n in w:
            assert torch.equal(g[n], w[n]), f"step {i}: {n}"
        for n in bst:
            assert torch.equal(g[n], bst[n]), f"step {i}: {n} against the best-class step"
        assert int(g["count"].min()) > 0 and not bool(g["range_flags"].any())
    for n in inline[0]:
        assert torch.equal(last[n], inline[0][n])
    want = "topn.topn_similarity_split" if (precision == "fp16x3" and k >= 256) else "topn.topn_rows"
    assert tr.calls.get(want, 0) == 7 and tr.calls.get("topn.topn_unpack", 0) == 7 and tr.calls.get("topn.topn_kept", 0) == 7
    assert tr.calls.get("best.nms_gather_labeled", 0) == 7 and "best.best_unpack" not in tr.calls and "lib.nms_gather" not in tr.calls
    _clean(tr)


def test_detector_keyword_gives_the_lists_per_box():
    from wedetect_amd import weights as W
    from wedetect_amd.detector import DetDataSample, YOLOWorldDetector
    sd_np = W.make_state_dict("nano")
    models = []
    for n_top in (0, 3):
        model = YOLOWorldDetector("nano", test_cfg=dict(max_per_img=50), max_classes=81, best_class=True, agnostic_nms=True, top_names=n_top)
        model.load_state_dict({"state_dict": {n: torch.from_numpy(v) for n, v in sd_np.items()}})
        model.cuda().eval()
        model.set_text_embeddings(torch.from_numpy(W.make_text_bank(81) * np.float32(2.5)))
        models.append(model)
    rgb = W.make_images(2, 128, 128, seed=77)
    bgr_chw = [torch.from_numpy(np.ascontiguousarray(im[..., ::-1].transpose(2, 0, 1))) for im in rgb]
    metas = [dict(ori_shape=(200, 256), scale_factor=(0.5, 0.5), pad_param=np.array([14., 14., 0., 0.])),
             dict(ori_shape=(128, 100), scale_factor=(1.0, 1.0), pad_param=np.array([0., 0., 14., 14.]))]
    batch = lambda: dict(inputs=bgr_chw, data_samples=[DetDataSample(metainfo=m) for m in metas])
    plain, res = models[0].test_step(batch()), models[1].test_step(batch())
    for p, r in zip(plain, res):
        pi, qi = r.pred_instances, p.pred_instances
        n = len(pi.scores)
        assert 0 < n <= 50 and tuple(pi.top_labels.shape) == (n, 3) and tuple(pi.top_scores.shape) == (n, 3)
        assert pi.top_labels.dtype == torch.int64 and "top_labels" not in qi
        assert torch.equal(pi.labels, qi.labels) and torch.equal(pi.scores, qi.scores) and torch.equal(pi.bboxes, qi.bboxes)
        assert torch.equal(pi.top_labels[:, 0], pi.labels) and torch.equal(pi.top_scores[:, 0], pi.scores)
        assert bool((pi.top_scores[:, :-1] >= pi.top_scores[:, 1:]).all()) and int(pi.top_labels.min()) >= 0 and int(pi.top_labels.max()) < 81
        assert all(len(set(row.tolist())) == 3 for row in pi.top_labels)
        kept = pi[pi.scores > pi.scores.median()]             # the lists travel with the rows through InstanceData's indexing
        assert tuple(kept.top_labels.shape) == (len(kept.scores), 3)
    with pytest.raises(NotImplementedError, match="top_names"):
        models[1].predict_tiled(np.zeros((300, 300, 3), np.uint8))


@pytest.mark.parametrize("k", [300, 4100])
def test_region_namer_names_every_valid_region(k):
    """N = 3 images of R = 37 regions, counts (37, 0, 5): the fused path against wd_topn_rows over the materialised logits (bit for
    bit), against float64 (scores within 2e-6, what wd_similarity_split is held to), regions from the count on empty; a planted 1e6
    embedding trips the guard and the fp32 path names the finite rows alike."""
    from wedetect_amd import lib as L
    from wedetect_amd import parallel as P
    from wedetect_amd import topn as TN
    from tests.test_gpu_split import _rand
    n_img, r, d, n = 3, 37, 768, 5
    rows = n_img * r
    e = _rand((rows, d), 501, 0.8).view(n_img, r, d)
    bank = torch.nn.functional.normalize(_rand((k, d), 502), dim=-1)
    g = torch.Generator().manual_seed(43)
    scales = (torch.rand(n_img, r, generator=g) * 1.5 + 0.2).cuda()
    bias = (torch.rand(n_img, r, generator=g) * 2 - 3).cuda()
    count = torch.tensor([37, 0, 5], device="cuda")
    valid = (torch.arange(r, device="cuda")[None, :] < count[:, None])
    namer = P.RegionNamer(bank, n)
    s, lab = namer(e, count, scales, bias)
    torch.cuda.synchronize()
    assert tuple(s.shape) == tuple(lab.shape) == (n_img, r, n) and s.dtype == torch.float32 and lab.dtype == torch.int32
    assert not namer.overflowed and namer.precision == "fp16x3"
    assert not bool(s[~valid].any()) and bool((lab[~valid] == -1).all()) and bool((lab[valid] >= 0).all())
    # the materialised path: the logits of the same split operands, then wd_topn_rows with the row affine
    es = torch.empty(L.LIB.wd_split_weights_bytes(rows, d), dtype=torch.uint8, device="cuda")
    L.split_weights_scaled(e.view(rows, d), es)
    ts = L.split_weights(bank)
    logits = torch.empty(rows, k, device="cuda")
    L.similarity_split(es, rows, ts[0], ts[1], logits, k, d, k, seg=(rows, rows, rows, (1.0, 1.0, 1.0), (0.0, 0.0, 0.0)), sigmoid=False)
    key = torch.zeros(rows, n, dtype=torch.int64, device="cuda")
    TN.topn_rows(logits, 1, rows, k, k, n, key, row_scale=scales.view(-1), row_bias=bias.view(-1))
    torch.cuda.synchronize()
    ws, wl = TN.unpack(key.cpu().numpy().view(np.uint64))
    v = valid.view(-1).cpu().numpy()
    assert np.array_equal(s.view(rows, n).cpu().numpy()[v].view(np.uint32), ws[v].view(np.uint32)) and np.array_equal(lab.view(rows, n).cpu().numpy()[v], wl[v])
    ref = torch.sigmoid((e.view(rows, d).double() @ bank.double().T) * scales.view(-1).double().exp()[:, None] + bias.view(-1).double()[:, None])
    top = ref.topk(n, dim=1).values
    err = float((s.view(rows, n).double() - top)[valid.view(-1)].abs().max())
    err_lab = float((torch.gather(ref, 1, lab.view(rows, n).long().clamp(min=0)) - top)[valid.view(-1)].abs().max())
    print(f"K {k}: max |score - float64| {err:.3g}, through the labels {err_lab:.3g}")
    assert err <= 2e-6 and err_lab <= 4e-6
    # the cached form gives the same
    s2, lab2 = P.device_region_names(e, count, scales, bias, bank, n)
    assert torch.equal(s2, s) and torch.equal(lab2, lab)
    P.clear_scorer_cache()
    # a planted 1e6 embedding: the guard trips, the namer switches to the fp32 path for good and repeats the call
    e2 = e.clone()
    e2[0, 3, 100] = 1e6
    with pytest.warns(UserWarning, match="fp32 path"):
        s3, lab3 = namer(e2, count, scales, bias)
    torch.cuda.synchronize()
    assert namer.overflowed and namer.precision == "fp32" and int(namer.flag) == 0
    keep = valid.clone()
    keep[0, 3] = False
    decided = ((top[:, :-1] - top[:, 1:]) > 4e-6).all(dim=1).view(n_img, r) & keep      # rankings the two arithmetics must share
    print(f"K {k}: rows whose float64 ranking decides the labels {int(decided.sum())}/{int(keep.sum())}")
    assert int(decided.sum()) >= int(keep.sum()) // 2        # a property of the float64 reference alone: the comparison below is not vacuous
    assert torch.equal(lab3[decided], lab[decided])
    assert float((s3[keep] - s[keep]).abs().max()) <= 4e-6
    assert not bool(s3[~valid].any()) and bool((lab3[~valid] == -1).all())


def test_infer_wedetect_dump_json_carries_the_names(tmp_path, monkeypatch):
    """infer_wedetect.main with --best-class and with --best-class --top-names 3 on one 320 x 320 image: the same detections, and
    per detection "names": [[name, score], ...] whose first entry is the drawn label."""
    import json
    import os

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
    for name, extra in (("best", ["--best-class"]), ("names", ["--best-class", "--top-names", "3"])):
        out_dir = str(tmp_path / name)
        res = iw.main(["--config", os.path.join(ROOT, "config", "wedetect_tiny.py"), "--checkpoint", ckpt_path, "--image", img_path,
                       "--text", str(tmp_path / "names.txt"), "--threshold", "0.05", "--topk", "100", "--device", "cuda:0",
                       "--output-dir", out_dir, "--dump-json", *extra], tokenizer=toy_tokenizer(vocab))
        assert len(res) == 1
        dumped[name] = json.load(open(os.path.join(out_dir, "synthetic.json")))
    names = dumped["names"].pop("names")
    assert "names" not in dumped["best"] and dumped["names"] == dumped["best"] and len(dumped["best"]["scores"]) > 0
    texts = dumped["best"]["texts"]
    assert len(names) == len(dumped["best"]["scores"])
    for lst, lab, sc in zip(names, dumped["best"]["labels"], dumped["best"]["scores"]):
        assert len(lst) == 3 and lst[0] == [texts[lab], sc] and len({n for n, _ in lst}) == 3
        assert lst[0][1] >= lst[1][1] >= lst[2][1] and all(n in texts for n, _ in lst)
