"""Box mAP without a GPU: hand-derived cases that pin the float64 restatement of pycocotools / lvis-api
(tests/det_eval_ref.py), the test datasets and metric configs, test.py's parser and refusals, the rank-0 gather of
predictions on a world-2 gloo group, and the match kernel's ISA (no scratch)."""
import importlib.util
import json
import os
import socket
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
import det_eval_ref as R  # noqa: E402


def _ann(gts, images=(1,), cats=(1,), lvis=False, img_extra=None):
    anns = []
    for n, g in enumerate(gts):
        a = dict(id=n + 1, image_id=g.get("image_id", 1), category_id=g.get("category_id", 1), bbox=g["bbox"],
                 area=g.get("area", g["bbox"][2] * g["bbox"][3]))
        if not lvis:
            a["iscrowd"] = g.get("iscrowd", 0)
        anns.append(a)
    ims = [dict(id=i, file_name=f"{i}.jpg", **((img_extra or {}).get(i, {}))) for i in images]
    cs = [dict(id=c, name=f"c{c}", **({"frequency": "f"} if lvis else {})) for c in cats]
    return dict(images=ims, annotations=anns, categories=cs)


def _dets(rows, image_id=1):
    """rows: (x1, y1, x2, y2, score, category)"""
    a = np.asarray(rows, np.float64).reshape(-1, 6)
    return [dict(image_id=image_id, bboxes=a[:, :4].astype(np.float32), scores=a[:, 4].astype(np.float32),
                 category_ids=a[:, 5].astype(np.int64))]


# pr = tp / (fp + tp + 2^-52): a lone TP has precision 1 / (1 + 2^-52), one ulp below 1, hence approx for "AP 1.0"
GT = dict(bbox=[10.0, 10.0, 50.0, 50.0])
TP = (10, 10, 60, 60)
FP = (200, 200, 240, 240)


def test_tp_before_fp_is_ap_1_and_fp_before_tp_is_ap_half():
    ev = R.coco_eval(_ann([GT]), _dets([(*TP, .9, 1), (*FP, .8, 1)]))
    assert ev["stats"][0] == pytest.approx(1.0) and ev["stats"][1] == pytest.approx(1.0)
    ev = R.coco_eval(_ann([GT]), _dets([(*FP, .9, 1), (*TP, .8, 1)]))
    assert ev["stats"][0] == pytest.approx(0.5)                               # pr = [0, .5] -> envelope [.5, .5]
    assert np.all(ev["precision"][:, :, 0, 0, 2] == 0.5) and np.all(ev["recall"][:, 0, 0, 2] == 1.0)


def test_det_on_crowd_gt_is_neither_tp_nor_fp():
    crowd = dict(bbox=[200.0, 200.0, 40.0, 40.0], iscrowd=1)
    ev = R.coco_eval(_ann([GT, crowd]), _dets([(*FP, .9, 1), (*TP, .8, 1)]))
    assert ev["stats"][0] == pytest.approx(1.0)                               # the det on the crowd box is ignored, not an FP
    ev = R.coco_eval(_ann([GT]), _dets([(*FP, .9, 1), (*TP, .8, 1)]))
    assert ev["stats"][0] == pytest.approx(0.5)


def test_area_range_follows_the_json_area_not_the_box():
    # a 50 x 50 box (2 500: medium by its box) whose JSON area is 500 (small)
    ev = R.coco_eval(_ann([dict(bbox=[10.0, 10.0, 50.0, 50.0], area=500.0)]), _dets([(*TP, .9, 1)]))
    assert ev["stats"][3] == pytest.approx(1.0)                               # small: the gt counts
    assert ev["stats"][4] == -1.0                              # medium: no kept gt -> -1
    assert np.all(ev["precision"][:, :, 0, 2, :] == -1)


def test_truncation_at_max_dets_happens_before_matching():
    rows = [(*FP, .9, 1), (*FP, .8, 1), (*FP, .7, 1), (*TP, .6, 1)]
    ev = R.coco_eval(_ann([GT]), _dets(rows), max_dets=(1, 2, 3))
    assert np.all(ev["recall"][:, 0, 0, :] == 0)               # the TP is 4th: cut at maxDets[-1] = 3
    ev = R.coco_eval(_ann([GT]), _dets(rows), max_dets=(1, 2, 4))
    assert np.all(ev["recall"][:, 0, 0, 2] == 1) and np.all(ev["recall"][:, 0, 0, 1] == 0)


def test_score_tie_keeps_the_stable_order():
    ev = R.coco_eval(_ann([GT]), _dets([(*FP, .5, 1), (*TP, .5, 1)]))
    assert ev["stats"][0] == pytest.approx(0.5)
    ev = R.coco_eval(_ann([GT]), _dets([(*TP, .5, 1), (*FP, .5, 1)]))
    assert ev["stats"][0] == pytest.approx(1.0)


def test_lvis_det_outside_pos_and_neg_is_dropped():
    extra = {1: dict(neg_category_ids=[], not_exhaustive_category_ids=[])}
    ann = _ann([GT], cats=(1, 2), lvis=True, img_extra=extra)
    ann["categories"][1]["frequency"] = "r"
    ev = R.lvis_eval(ann, _dets([(*FP, .9, 2), (*TP, .8, 1)]))
    assert ev["stats"][0] == pytest.approx(1.0)                               # category 2 is neither in the image nor negative: dropped
    extra[1]["neg_category_ids"] = [2]
    ann2 = _ann([GT], cats=(1, 2), lvis=True, img_extra=extra)
    ann2["categories"][1]["frequency"] = "r"
    ev = R.lvis_eval(ann2, _dets([(*FP, .9, 2), (*TP, .8, 1)]))
    assert ev["stats"][0] == pytest.approx(1.0)                               # kept, but category 2 has no gt: its AP is -1, not counted
    assert np.all(ev["precision"][:, :, 1, :] == -1)


def test_lvis_unmatched_det_in_not_exhaustive_category_is_ignored():
    extra = {1: dict(neg_category_ids=[], not_exhaustive_category_ids=[1])}
    ev = R.lvis_eval(_ann([GT], lvis=True, img_extra=extra), _dets([(*FP, .9, 1), (*TP, .8, 1)]))
    assert ev["stats"][0] == pytest.approx(1.0)
    extra[1]["not_exhaustive_category_ids"] = []
    ev = R.lvis_eval(_ann([GT], lvis=True, img_extra=extra), _dets([(*FP, .9, 1), (*TP, .8, 1)]))
    assert ev["stats"][0] == pytest.approx(0.5)


def test_lvis_per_image_limit_is_across_categories():
    extra = {1: dict(neg_category_ids=[2], not_exhaustive_category_ids=[])}
    ann = _ann([GT], cats=(1, 2), lvis=True, img_extra=extra)
    rows = [(*FP, .9, 2), (*FP, .85, 2), (*TP, .8, 1)]
    assert R.lvis_eval(ann, _dets(rows), max_dets=3)["stats"][0] == pytest.approx(1.0)
    assert R.lvis_eval(ann, _dets(rows), max_dets=2)["stats"][0] == pytest.approx(0.0)   # the TP is the 3rd of the image


def test_lvis_frequency_groups():
    gts = [dict(bbox=[10.0, 10.0, 50.0, 50.0], category_id=c) for c in (1, 2, 3)]
    ann = _ann(gts, cats=(1, 2, 3), lvis=True, img_extra={1: dict(neg_category_ids=[], not_exhaustive_category_ids=[])})
    for c, f in zip(ann["categories"], "rcf"):
        c["frequency"] = f
    ev = R.lvis_eval(ann, _dets([(*TP, .9, 1), (*FP, .95, 2), (*TP, .9, 2), (*FP, .9, 3)]))
    assert ev["freq_groups"] == [[0], [1], [2]]
    assert ev["stats"][6] == pytest.approx(1.0) and ev["stats"][7] == pytest.approx(0.5) and ev["stats"][8] == pytest.approx(0.0)
    assert ev["stats"][0] == pytest.approx(0.5)


def test_headline_ap_is_at_100_dets_per_pair():
    """pycocotools _summarizeDets: stats[0] = _summarize(1) keeps maxDets=100 although mmdet sets maxDets to
    (100, 300, 1000); AP50 / AP75 / AP s/m/l are at 1000.  One pair with 100 FPs above its only TP: AP@100 is 0."""
    rows = [(200 + i, 200, 240 + i, 240, .9 - i * 1e-3, 1) for i in range(100)] + [(*TP, .5, 1)]
    ev = R.coco_eval(_ann([GT]), _dets(rows))
    assert ev["stats"][0] == 0.0                                         # AP@100: the TP is the 101st det
    at_1000 = ev["precision"][:, :, :, 0, 2]
    assert at_1000.mean() == pytest.approx(1 / 101)                    # the same mean at maxDets 1000 is not 0
    assert ev["stats"][1] == pytest.approx(1 / 101)                    # AP50 is at 1000
    assert ev["stats"][6] == 0.0 and ev["stats"][8] == 1.0             # AR@100, AR@1000


def test_metric_lines_follow_the_libraries_format():
    from wedetect_amd.datasets import metric_lines
    lines = metric_lines(dict(stats=np.linspace(0, 1, 12)), lvis=False)
    assert lines[0] == " Average Precision  (AP) @[ IoU=0.50:0.95 | area=   all | maxDets=100 ] = 0.000"
    assert lines[1] == " Average Precision  (AP) @[ IoU=0.50      | area=   all | maxDets=1000 ] = 0.091"
    assert lines[7] == " Average Recall     (AR) @[ IoU=0.50:0.95 | area=   all | maxDets=300 ] = 0.636"
    lines = metric_lines(dict(stats=np.linspace(0, 1, 13)), lvis=True)
    assert lines[1] == " Average Precision  (AP) @[ IoU=0.50      | area=   all | maxDets=300 catIds=all] = 0.083"
    assert lines[3] == " Average Precision  (AP) @[ IoU=0.50:0.95 | area=     s | maxDets=300 catIds=all] = 0.250"
    assert lines[6] == " Average Precision  (AP) @[ IoU=0.50:0.95 | area=   all | maxDets=300 catIds=  r] = 0.500"
    assert lines[9] == " Average Recall     (AR) @[ IoU=0.50:0.95 | area=   all | maxDets=300 catIds=all] = 0.750"


def test_restatement_matches_pycocotools_when_installed():
    pytest.importorskip("pycocotools")
    from pycocotools.coco import COCO
    from pycocotools.cocoeval import COCOeval
    ann, dets = R.make_set(0, n_img=30, n_cat=5, extra=[(3, 1, 150, 4)])
    gt = COCO()
    gt.dataset = json.loads(json.dumps(ann))
    gt.createIndex()
    dt = gt.loadRes(R.results_list(dets))
    e = COCOeval(gt, dt, "bbox")
    e.params.maxDets = [100, 300, 1000]
    e.evaluate()
    e.accumulate()
    e.summarize()
    ref = R.coco_eval(ann, dets)
    for key in ("precision", "recall", "scores"):
        assert np.array_equal(e.eval[key], ref[key]), key
    assert np.array_equal(np.asarray(e.stats, np.float64), ref["stats"])


def test_restatement_matches_lvis_api_when_installed(tmp_path):
    pytest.importorskip("lvis")
    from lvis import LVIS, LVISEval, LVISResults
    ann, dets = R.make_set(1, n_img=30, n_cat=6, lvis=True, extra=[(2, 0, 400, 5)])
    (tmp_path / "lvis.json").write_text(json.dumps(ann))
    gt = LVIS(str(tmp_path / "lvis.json"))
    res = LVISResults(gt, R.results_list(dets), max_dets=300)
    e = LVISEval(gt, res, "bbox")
    e.run()
    ref = R.lvis_eval(ann, dets)
    assert np.array_equal(e.eval["precision"], ref["precision"]) and np.array_equal(e.eval["recall"], ref["recall"])
    from wedetect_amd.det_eval import LVIS_STAT_NAMES
    assert [e.results[k] for k in LVIS_STAT_NAMES] == ref["stats"].tolist()


# ------------------------------------------------------------------------------------------ host layer
def test_match_workspace_formula_matches_the_library():
    from wedetect_amd import lib as L
    for dk, g in ((0, 0), (1, 1), (3, 5), (1000, 33), (7, 120)):
        need = 8 * dk * g + 4 * dk + 4 * 40 * ((g + 31) // 32) + g
        assert int(L.LIB.wd_det_match_workspace_bytes(dk, g)) == (need + 15) & ~15
    assert int(L.LIB.wd_det_match_lds_bytes()) == 8192


def test_match_kernel_isa_has_no_scratch(tmp_path):
    from wedetect_amd import build as wb
    asm = str(tmp_path / "det_eval.s")
    cmd = [wb.HIPCC, *[f for f in wb.FLAGS if f != "-fPIC"], "-S", "--cuda-device-only",
           os.path.join(wb.CSRC, "det_eval.hip"), "-o", asm]
    subprocess.check_call(cmd, stderr=subprocess.DEVNULL)
    meta = open(asm).read()
    meta = meta[meta.index("amdhsa.kernels"):]
    seen = 0
    for blk in meta.split("- .agpr_count")[1:]:
        if "det_match_kernel" in blk or "det_accumulate_kernel" in blk:
            seen += 1
            assert "private_segment_fixed_size: 0\n" in blk
            assert "vgpr_spill_count: 0\n" in blk and "sgpr_spill_count: 0\n" in blk
    assert seen == 2


def test_lvis_keep_mask():
    from wedetect_amd.det_eval import lvis_keep
    ann = dict(images=[dict(id=1, neg_category_ids=[3]), dict(id=2, neg_category_ids=[])],
               annotations=[dict(image_id=1, category_id=2)], categories=[dict(id=2), dict(id=3), dict(id=4)])
    img = np.array([1, 1, 1, 1, 2, 9])
    cat = np.array([2, 3, 4, 2, 2, 2])
    score = np.array([.5, .5, .9, .5, .9, .9], np.float32)
    keep = lvis_keep(ann, img, cat, score, max_dets=2)
    # image 1: top-2 by score (stable) are rows 2 (.9) and 0 (.5); row 2's category is outside pos | neg
    assert keep.tolist() == [True, False, False, False, False, False]


def _write_coco(tmp_path, lvis=False):
    images = [dict(id=30, width=64, height=48), dict(id=7, width=64, height=48), dict(id=12, width=64, height=48)]
    for im in images:
        if lvis:
            im["coco_url"] = f"http://images.cocodataset.org/val2017/{im['id']:012d}.jpg"
        else:
            im["file_name"] = f"{im['id']:012d}.jpg"
    cats = [dict(id=9, name="kite"), dict(id=2, name="dog"), dict(id=5, name="cup")]
    ann = dict(images=images, annotations=[], categories=cats)
    p = tmp_path / "ann.json"
    p.write_text(json.dumps(ann))
    t = tmp_path / "texts.json"
    t.write_text(json.dumps([["a dog"], ["a cup"], ["a kite"]]))
    return str(p), str(t)


@pytest.mark.parametrize("lvis", [False, True])
def test_datasets_order_labels_and_texts(tmp_path, lvis):
    from wedetect_amd.registry import DATASETS
    from wedetect_amd import config as _config  # noqa: F401  (fills the registries)
    ann, texts = _write_coco(tmp_path, lvis)
    ds = DATASETS.build(dict(type="MultiModalDataset", class_text_path=texts, pipeline=[],
                             dataset=dict(type="YOLOv5LVISV1Dataset" if lvis else "WeCocoDataset", data_root=str(tmp_path),
                                          ann_file="ann.json", test_mode=True, batch_shapes_cfg=None,
                                          data_prefix=dict(img="" if lvis else "val2017"))))
    assert len(ds) == 3
    infos = [ds.get_data_info(i) for i in range(3)]
    assert [i["img_id"] for i in infos] == [30, 7, 12]                     # annotation-file order
    # COCO: data_prefix val2017 + file_name; LVIS: empty prefix + coco_url without the host ("val2017/...")
    assert os.path.normpath(infos[1]["img_path"]) == os.path.join(str(tmp_path), "val2017", "000000000007.jpg")
    assert infos[0]["texts"] == [["a dog"], ["a cup"], ["a kite"]]
    assert ds.metainfo["classes"] == ("dog", "cup", "kite")               # ascending category id
    assert ds.dataset.cat_ids == [2, 5, 9]


def test_datasets_refuse_training_mode(tmp_path):
    from wedetect_amd.datasets import WeCocoDataset
    ann, _ = _write_coco(tmp_path)
    with pytest.raises(NotImplementedError, match="test_mode"):
        WeCocoDataset(ann_file=ann, test_mode=False)


def test_metric_configs_refuse_unsupported_options(tmp_path):
    from wedetect_amd.registry import METRICS
    from wedetect_amd import config as _config  # noqa: F401
    for bad, what in ((dict(metric="segm"), "segm"), (dict(metric=["bbox", "proposal"]), "proposal"),
                      (dict(iou_thrs=[0.5]), "iou_thrs"), (dict(format_only=True), "outfile_prefix")):
        for t in ("CocoMetric", "LVISMetric"):
            with pytest.raises((NotImplementedError, ValueError), match=what):
                METRICS.build(dict(type=t, ann_file="x.json", **bad))
    m = METRICS.build(dict(type="CocoMetric", ann_file="x.json", metric="bbox", iou_thrs=list(np.linspace(.5, .95, 10))))
    ann = dict(images=[dict(id=4)], annotations=[], categories=[dict(id=8, name="a"), dict(id=3, name="b")])
    m.process([dict(img_id=4, bboxes=np.array([[1, 2, 5, 9]], np.float32), scores=np.array([.5], np.float32),
                    labels=np.array([1]))])
    d = m.dets(ann)
    assert d[0]["category_ids"].tolist() == [8]                            # label 1 -> second-smallest id
    path = m.write_results(d, str(tmp_path / "out" / "res"))
    rec = json.load(open(path))
    assert path.endswith("res.bbox.json") and rec == [dict(image_id=4, bbox=[1.0, 2.0, 4.0, 7.0], score=0.5, category_id=8)]


def test_tiny_config_carries_the_evaluation_sections():
    from wedetect_amd.cfgfile import Config
    for size in ("tiny", "base", "large"):
        cfg = Config.fromfile(os.path.join(ROOT, "config", f"wedetect_{size}.py"))
        assert cfg.test_evaluator.type == "CocoMetric" and cfg.test_evaluator.metric == "bbox"
        assert cfg.test_dataloader.dataset.dataset.type == "WeCocoDataset"
        assert cfg.lvis_minival_evaluator.type == "LVISMetric"
        assert cfg.test_dataloader.dataset.pipeline == cfg.test_pipeline   # large: its 1280 pipeline


# ------------------------------------------------------------------------------------------ test.py
def _entry():
    spec = importlib.util.spec_from_file_location("wd_test_entry", os.path.join(ROOT, "test.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_test_py_parser_takes_the_reference_flags():
    T = _entry()
    a = T.parse_args(["c.py", "k.pth", "--work-dir", "w", "--out", "p.pkl", "--launcher", "pytorch", "--local-rank", "3",
                      "--cfg-options", "test_dataloader.batch_size=2", "--text-bank", "b.pt", "--precision", "fp32"])
    assert (a.config, a.checkpoint, a.work_dir, a.out, a.launcher, a.local_rank) == ("c.py", "k.pth", "w", "p.pkl", "pytorch", 3)
    assert a.cfg_options == {"test_dataloader.batch_size": 2} and a.text_bank == "b.pt" and a.precision == "fp32"
    assert T.parse_args(["c.py", "k.pth", "--local_rank", "1"]).local_rank == 1


@pytest.mark.parametrize("flags", [["--show"], ["--show-dir", "d"], ["--tta"], ["--launcher", "slurm"], ["--out", "x.json"]])
def test_test_py_refuses_out_of_scope_flags(flags, capsys):
    T = _entry()
    with pytest.raises(SystemExit) as e:
        T.parse_args(["c.py", "k.pth", *flags])
    assert e.value.code == 2
    err = capsys.readouterr().err
    assert "not implemented" in err or "pkl" in err


def test_dist_test_sh_interface():
    src = open(os.path.join(ROOT, "dist_test.sh")).read()
    for v in ("NNODES", "NODE_RANK", "PORT", "MASTER_ADDR", "--nproc_per_node", "--launcher pytorch"):
        assert v in src
    p = subprocess.run(["bash", os.path.join(ROOT, "dist_test.sh")], capture_output=True, text=True, timeout=30)
    assert p.returncode == 2 and "usage" in p.stderr


# ------------------------------------------------------------------------------------------ rank-0 gather
def _gather_worker(rank, world, port, shards, q):
    import torch.distributed as dist
    from wedetect_amd.parallel import gather_to_rank0
    dist.init_process_group("gloo", init_method=f"tcp://127.0.0.1:{port}", rank=rank, world_size=world)
    try:
        got = gather_to_rank0(shards[rank])
        q.put((rank, got))
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize("shards", [[[dict(img_id=1, s=np.arange(3))], [dict(img_id=2), dict(img_id=3)]],
                                    [[], [dict(img_id=5)]], [[dict(img_id=4)], []], [[], []]])
def test_gather_predictions_to_rank0_on_gloo(shards):
    import multiprocessing as mp
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    ps = [ctx.Process(target=_gather_worker, args=(r, 2, port, shards, q)) for r in range(2)]
    for p in ps:
        p.start()
    res = dict(q.get(timeout=120) for _ in ps)
    for p in ps:
        p.join(timeout=60)
        assert p.exitcode == 0
    assert res[1] is None
    flat = shards[0] + shards[1]
    assert [r["img_id"] for r in res[0]] == [r["img_id"] for r in flat]
    if flat and "s" in flat[0]:
        assert np.array_equal(res[0][0]["s"], np.arange(3))


def test_gather_without_process_group_is_identity():
    from wedetect_amd.parallel import gather_to_rank0
    assert gather_to_rank0([1, 2]) == [1, 2]
