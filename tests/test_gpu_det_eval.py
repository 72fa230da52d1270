"""Device COCO / LVIS box mAP (wedetect_amd.det_eval) against the float64 restatement of pycocotools / lvis-api
(tests/det_eval_ref.py): precision, recall, scores and every stat equal by np.array_equal on seeded synthetic sets."""
import json
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import det_eval_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu


def _det_eval():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("needs a HIP device")
    from wedetect_amd import det_eval
    return det_eval


def _same_coco(ann, dets):
    de = _det_eval()
    got = de.coco_evaluate(ann, dets)
    ref = R.coco_eval(ann, dets)
    for k in ("precision", "recall", "scores", "stats"):
        assert got[k].shape == ref[k].shape, k
        assert np.array_equal(got[k], ref[k]), (k, np.argwhere(got[k] != ref[k])[:5])
    return got


def _same_lvis(ann, dets):
    de = _det_eval()
    got = de.lvis_evaluate(ann, dets)
    ref = R.lvis_eval(ann, dets)
    for k in ("precision", "recall", "stats"):
        assert got[k].shape == ref[k].shape, k
        assert np.array_equal(got[k], ref[k]), (k, np.argwhere(got[k] != ref[k])[:5])
    return got


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_coco_small_sets_equal_restatement(seed):
    ann, dets = R.make_set(seed, n_img=60, n_cat=7, crowd_frac=0.15, empty_frac=0.15, no_det_frac=0.15)
    got = _same_coco(ann, dets)
    assert got["stats"][0] > 0                                # the set is not degenerate
    assert set(got["metrics"]) >= {"bbox_mAP", "bbox_mAP_50", "bbox_mAP_75", "bbox_mAP_s", "bbox_mAP_m", "bbox_mAP_l",
                                   "bbox_mAP_copypaste"}


def test_coco_score_ties():
    ann, dets = R.make_set(11, n_img=50, n_cat=5, tie_levels=4, dets_per_img=60)
    _same_coco(ann, dets)


def test_coco_truncation_and_large_pairs():
    # image 3, category 1: 1 300 dets (truncated at 1 000 before matching); image 5, category 2: 120 gts x 300 dets
    # (far past the LDS slice of a pair: global scratch); category 1 spans many 256-det chunks
    ann, dets = R.make_set(12, n_img=30, n_cat=4, extra=[(3, 1, 1300, 6), (5, 2, 300, 120), (7, 1, 900, 3)])
    _same_coco(ann, dets)


def test_coco_headline_ap_at_100_dets():
    # one pair with 100 FPs ranked above its only TP: bbox_mAP (AP@100) is 0 while AP50 (at 1000) is not
    ann = dict(images=[dict(id=1)], categories=[dict(id=1, name="a")],
               annotations=[dict(id=1, image_id=1, category_id=1, bbox=[10.0, 10.0, 50.0, 50.0], area=2500.0, iscrowd=0)])
    boxes = np.array([[200 + i, 200, 240 + i, 240] for i in range(100)] + [[10, 10, 60, 60]], np.float32)
    scores = np.array([.9 - i * 1e-3 for i in range(100)] + [.5], np.float32)
    got = _same_coco(ann, [dict(image_id=1, bboxes=boxes, scores=scores, category_ids=np.ones(101, np.int64))])
    assert got["stats"][0] == 0.0 and got["stats"][1] > 0 and got["metrics"]["bbox_mAP"] == 0.0


def test_coco_signed_zero_scores_tie():
    # -0.0 and +0.0 compare equal: the stable (image, rank) order decides, as in numpy's mergesort
    ann, dets = R.make_set(14, n_img=20, n_cat=3, dets_per_img=20)
    for n, d in enumerate(dets):
        s = d["scores"].copy()
        s[::2] = -0.0 if n % 2 else 0.0
        d["scores"] = s
    _same_coco(ann, dets)


def test_coco_gt_without_dets_and_no_dets_at_all():
    ann, dets = R.make_set(13, n_img=20, n_cat=4)
    _same_coco(ann, [])
    _same_coco(ann, dets[:3])


@pytest.mark.parametrize("seed", [0, 1])
def test_lvis_sets_equal_restatement(seed):
    ann, dets = R.make_set(20 + seed, n_img=60, n_cat=9, lvis=True, dets_per_img=80)
    got = _same_lvis(ann, dets)
    assert set(got["metrics"]) == {f"bbox_{n}" for n in ("AP", "AP50", "AP75", "APs", "APm", "APl", "APr", "APc", "APf")}


def test_lvis_per_image_limit_and_ties():
    # 700 dets on one image: LVISResults keeps the 300 best (stable); quantised scores tie across the cut
    ann, dets = R.make_set(30, n_img=25, n_cat=6, lvis=True, tie_levels=8, extra=[(2, 0, 700, 5), (4, 1, 260, 90)])
    _same_lvis(ann, dets)


def test_coco_val_scale():
    """5 000 images, 80 classes, 300 dets per image (1.5 M dets, 1 000-det truncation inactive)."""
    ann, dets = R.make_set(5, n_img=5000, n_cat=80, dets_per_img=300, fixed_dets=True, gts_per_img=(0, 14),
                           no_det_frac=0.02, empty_frac=0.02)
    _same_coco(ann, dets)


# ------------------------------------------------------------------------------------------ test.py end to end
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _write_dataset(tmp, lvis):
    from PIL import Image
    rng = np.random.default_rng(7)
    names = ["person", "dog", "kite", "cup", "chair"]
    cat_ids = [3, 1, 18, 44, 62]
    (tmp / "val").mkdir(exist_ok=True)
    images, anns = [], []
    for n in range(12):
        h, w = int(rng.integers(96, 200)), int(rng.integers(96, 200))
        iid = 1000 - 37 * n
        Image.fromarray(rng.integers(0, 256, (h, w, 3), dtype=np.uint8)).save(tmp / "val" / f"{iid}.jpg", quality=95)
        im = dict(id=iid, width=w, height=h)
        if lvis:
            im["coco_url"] = f"http://images.cocodataset.org/val/{iid}.jpg"
            im["neg_category_ids"] = [cat_ids[int(rng.integers(0, 5))]]
            im["not_exhaustive_category_ids"] = []
        else:
            im["file_name"] = f"{iid}.jpg"
        images.append(im)
        for _ in range(int(rng.integers(0, 4))):
            x, y = float(rng.uniform(0, w - 20)), float(rng.uniform(0, h - 20))
            bw, bh = float(rng.uniform(8, w - x)), float(rng.uniform(8, h - y))
            a = dict(id=len(anns) + 1, image_id=iid, category_id=cat_ids[int(rng.integers(0, 5))], bbox=[x, y, bw, bh],
                     area=bw * bh)
            if not lvis:
                a["iscrowd"] = 0
            anns.append(a)
    cats = [dict(id=c, name=nm) for c, nm in zip(cat_ids, names)]
    if lvis:
        for k, c in enumerate(cats):
            c["frequency"] = "rcf"[k % 3]
    ann = dict(images=images, annotations=anns, categories=cats)
    path = tmp / ("lvis.json" if lvis else "coco.json")
    path.write_text(json.dumps(ann))
    texts = tmp / "texts.json"
    texts.write_text(json.dumps([[nm] for _, nm in sorted(zip(cat_ids, names))]))
    return ann, str(path), str(texts)


@pytest.mark.parametrize("lvis", [False, True])
def test_test_py_end_to_end(tmp_path, lvis):
    import pickle
    import subprocess
    import torch
    from wedetect_amd import weights as W

    ann, ann_path, texts_path = _write_dataset(tmp_path, lvis)
    sd = {k: torch.from_numpy(v) for k, v in W.make_state_dict("tiny").items()}
    ckpt = str(tmp_path / "tiny.pth")
    torch.save({"state_dict": sd, "meta": {}}, ckpt)
    bank = torch.from_numpy(np.random.default_rng(3).standard_normal((5, 768)).astype(np.float32))
    bank_path = str(tmp_path / "bank.pt")
    torch.save(bank, bank_path)
    ds = "YOLOv5LVISV1Dataset" if lvis else "WeCocoDataset"
    opts = [f"test_dataloader.dataset.dataset.type={ds}", f"test_dataloader.dataset.dataset.data_root={tmp_path}/",
            f"test_dataloader.dataset.dataset.ann_file={ann_path}",
            f"test_dataloader.dataset.dataset.data_prefix.img={'' if lvis else 'val'}",
            f"test_dataloader.dataset.class_text_path={texts_path}",
            f"test_evaluator.type={'LVISMetric' if lvis else 'CocoMetric'}", f"test_evaluator.ann_file={ann_path}"]
    out = str(tmp_path / "preds.pkl")
    cmd = [sys.executable, os.path.join(ROOT, "test.py"), os.path.join(ROOT, "config", "wedetect_tiny.py"), ckpt,
           "--text-bank", bank_path, "--out", out, "--work-dir", str(tmp_path / "wd"), "--cfg-options", *opts]
    p = subprocess.run(cmd, capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert p.returncode == 0, p.stdout[-3000:] + p.stderr[-3000:]
    preds = pickle.load(open(out, "rb"))
    assert [q["img_id"] for q in preds] == [im["id"] for im in ann["images"]]          # annotation-file order
    # the predictions equal test_step on the same images
    from wedetect_amd.apis import init_detector
    from wedetect_amd.cfgfile import Config
    from wedetect_amd.datasets import build_dataset
    cfg = Config.fromfile(os.path.join(ROOT, "config", "wedetect_tiny.py"))
    cfg.merge_from_dict(dict(o.split("=", 1) for o in opts))
    dset = build_dataset(cfg.test_dataloader.dataset)
    model = init_detector(cfg, ckpt, device="cuda:0")
    model.set_text_embeddings(bank.cuda(), dset.class_texts)
    for i, q in enumerate(preds):
        item = dset[i]
        o = model.test_step(dict(inputs=item["inputs"].unsqueeze(0), data_samples=[item["data_samples"]]))[0].pred_instances
        for key in ("bboxes", "scores", "labels"):
            assert torch.equal(getattr(o, key).cpu(), q["pred_instances"][key].to(getattr(o, key).dtype)), key
    assert sum(len(q["pred_instances"]["scores"]) for q in preds) > 0
    # the printed metrics equal the restatement on those predictions
    cat_ids = np.asarray(sorted(c["id"] for c in ann["categories"]))
    dets = [dict(image_id=q["img_id"], bboxes=q["pred_instances"]["bboxes"].numpy(),
                 scores=q["pred_instances"]["scores"].numpy(),
                 category_ids=cat_ids[q["pred_instances"]["labels"].numpy()]) for q in preds]
    ref = R.lvis_eval(ann, dets) if lvis else R.coco_eval(ann, dets)
    metrics = json.load(open(tmp_path / "wd" / "metrics.json"))
    names = (["AP", "AP50", "AP75", "APs", "APm", "APl", "APr", "APc", "APf"] if lvis
             else ["mAP", "mAP_50", "mAP_75", "mAP_s", "mAP_m", "mAP_l"])
    for n, v in zip(names, ref["stats"]):
        assert metrics[f"bbox_{n}"] == float(f"{round(float(v), 3)}"), n
    # every summary line, in the libraries' format, with the restatement's values (AR@300 and APr/c/f for LVIS)
    from wedetect_amd.datasets import metric_lines
    for line in metric_lines(dict(stats=ref["stats"]), lvis):
        assert line + "\n" in p.stdout, line
    if lvis:
        assert "maxDets=300 catIds=  r]" in p.stdout and " Average Recall     (AR) @[ IoU=0.50:0.95 | area=   all | maxDets=300 catIds=all]" in p.stdout
    else:
        assert " Average Precision  (AP) @[ IoU=0.50:0.95 | area=   all | maxDets=100 ] = " in p.stdout
        assert "bbox_mAP_copypaste" in metrics
