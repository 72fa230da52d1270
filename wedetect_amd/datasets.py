"""Test-mode datasets and box-mAP metrics behind the config's ``test_dataloader`` / ``test_evaluator`` (host Python).

* ``WeCocoDataset`` / ``YOLOv5LVISV1Dataset``: the images of a COCO- / LVIS-format annotation file in file order, no
  filtering (test mode).  ``ann_file`` and ``data_prefix['img']`` are joined to ``data_root`` when relative, as
  mmengine's BaseDataset does; an LVIS image's path is its ``file_name``, or its ``coco_url`` without the
  ``http://images.cocodataset.org/`` prefix.  ``classes`` are the category names in ascending id order: label k is
  the k-th of them (``cat_ids[k]``).
* ``MultiModalDataset``: wraps one of them, adds ``texts`` (the JSON list of ``class_text_path``, one list of captions
  per class) to every item and runs the test pipeline.
* ``CocoMetric`` / ``LVISMetric``: collect per-image predictions (``process``) and evaluate them with
  :mod:`wedetect_amd.det_eval` (``compute_metrics``).  Options outside box mAP raise by name.
"""
from __future__ import annotations

import json
import os
import os.path as osp
from typing import Dict, List, Optional, Sequence

import numpy as np

from .registry import DATASETS, METRICS

_COCO_URL = "http://images.cocodataset.org/"


def _join(root: Optional[str], path: Optional[str]) -> str:
    if path is None:
        return root or ""
    if root and not osp.isabs(path):
        return osp.join(root, path)
    return path


def load_annotations(path: str) -> dict:
    with open(path) as f:
        return json.load(f)


class _AnnDataset:
    lvis = False

    def __init__(self, ann_file: str, data_root: Optional[str] = None, data_prefix: Optional[dict] = None,
                 test_mode: bool = True, metainfo: Optional[dict] = None, pipeline: Sequence = (),
                 batch_shapes_cfg=None, filter_cfg=None, debug_mode: bool = False, backend_args=None, **kwargs):
        if not test_mode:
            raise NotImplementedError(f"{type(self).__name__}: only test_mode=True (evaluation) is implemented")
        if batch_shapes_cfg is not None:
            raise NotImplementedError(f"{type(self).__name__}: batch_shapes_cfg is not implemented (the configs set None)")
        if pipeline:
            raise NotImplementedError(f"{type(self).__name__}: give the pipeline to MultiModalDataset")
        unknown = sorted(set(kwargs) - {"lazy_init", "serialize_data", "indices", "max_refetch", "return_classes"})
        if unknown:
            raise TypeError(f"{type(self).__name__}: unsupported options {unknown}")
        self.data_root = data_root
        self.ann_file = _join(data_root, ann_file)
        self.img_prefix = _join(data_root, (data_prefix or {}).get("img", ""))
        self.test_mode = True
        self.debug_mode = debug_mode
        self.ann = load_annotations(self.ann_file)
        cats = sorted(self.ann.get("categories", []), key=lambda c: c["id"])
        self.cat_ids = [int(c["id"]) for c in cats]
        classes = tuple(c.get("name", str(c["id"])) for c in cats)
        meta = dict(metainfo or {})
        if isinstance(meta.get("classes"), str) and osp.isfile(meta["classes"]):
            with open(meta["classes"]) as f:
                meta["classes"] = json.load(f)
        meta.setdefault("classes", classes)
        self.metainfo = meta
        self.data_list = [self._info(im) for im in self.ann.get("images", [])]

    def _info(self, im: dict) -> dict:
        if "file_name" in im:
            name = im["file_name"]
        elif "coco_url" in im:
            name = im["coco_url"].replace(_COCO_URL, "")
        else:
            raise KeyError(f"image {im.get('id')} has neither file_name nor coco_url")
        return dict(img_id=int(im["id"]), img_path=osp.join(self.img_prefix, name), height=im.get("height"),
                    width=im.get("width"))

    def __len__(self) -> int:
        return min(len(self.data_list), 100) if self.debug_mode else len(self.data_list)

    def get_data_info(self, idx: int) -> dict:
        return dict(self.data_list[idx])

    def full_init(self) -> None:
        pass


@DATASETS.register_module()
class WeCocoDataset(_AnnDataset):
    """COCO-format annotation file (mmdet CocoDataset / YOLOv5CocoDataset in test mode)."""


@DATASETS.register_module()
class YOLOv5LVISV1Dataset(_AnnDataset):
    """LVIS v1-format annotation file (mmdet LVISV1Dataset in test mode)."""
    lvis = True


@DATASETS.register_module()
class MultiModalDataset:
    """Dataset + class texts + test pipeline."""

    def __init__(self, dataset, class_text_path: Optional[str] = None, test_mode: bool = True,
                 pipeline: Sequence = (), lazy_init: bool = False):
        from .pipeline import Compose
        self.dataset = DATASETS.build(dataset) if isinstance(dataset, dict) else dataset
        if class_text_path is not None:
            with open(class_text_path) as f:
                self.class_texts = json.load(f)
        else:
            self.class_texts = None
        self.test_mode = test_mode
        self.pipeline = Compose(pipeline)

    @property
    def metainfo(self) -> dict:
        return dict(self.dataset.metainfo)

    def __len__(self) -> int:
        return len(self.dataset)

    def get_data_info(self, idx: int) -> dict:
        info = self.dataset.get_data_info(idx)
        if self.class_texts is not None:
            info["texts"] = self.class_texts
        return info

    def __getitem__(self, idx: int):
        return self.pipeline(self.get_data_info(idx))


def build_dataset(cfg) -> MultiModalDataset:
    return DATASETS.build(cfg.to_dict() if hasattr(cfg, "to_dict") else dict(cfg))


# ------------------------------------------------------------------------------------------ metrics
class _BoxMetric:
    lvis = False
    default_prefix = ""

    def __init__(self, ann_file: Optional[str] = None, metric="bbox", classwise: bool = False,
                 proposal_nums=None, iou_thrs=None, metric_items=None, format_only: bool = False,
                 outfile_prefix: Optional[str] = None, backend_args=None, collect_device: str = "cpu",
                 prefix: Optional[str] = None, sort_categories: bool = False, use_mp_eval: bool = False, **kwargs):
        name = type(self).__name__
        metrics = [metric] if isinstance(metric, str) else list(metric)
        bad = [m for m in metrics if m != "bbox"]
        if bad:
            raise NotImplementedError(f"{name}: metric {bad} is not implemented (box mAP only: metric='bbox')")
        if iou_thrs is not None and not np.array_equal(np.asarray(iou_thrs, np.float64), _default_iou_thrs()):
            raise NotImplementedError(f"{name}: iou_thrs other than linspace(.5, .95, 10) is not implemented")
        if not self.lvis and proposal_nums is not None and tuple(proposal_nums) != (100, 300, 1000):
            raise NotImplementedError(f"{name}: proposal_nums other than (100, 300, 1000) is not implemented")
        if format_only and outfile_prefix is None:
            raise ValueError(f"{name}: format_only needs outfile_prefix")
        if metric_items is not None:
            raise NotImplementedError(f"{name}: metric_items is not implemented (the default items are reported)")
        if kwargs:
            raise TypeError(f"{name}: unsupported options {sorted(kwargs)}")
        self.ann_file = ann_file
        self.classwise = classwise
        self.format_only = format_only
        self.outfile_prefix = outfile_prefix
        self.results: List[dict] = []
        self.dataset_meta: Dict = {}

    def process(self, preds: Sequence[dict]) -> None:
        """preds: dicts with ``img_id``, ``bboxes`` [n, 4] xyxy, ``scores`` [n], ``labels`` [n] (numpy or tensors)."""
        for p in preds:
            self.results.append(dict(img_id=int(p["img_id"]), bboxes=np.asarray(p["bboxes"], np.float32).reshape(-1, 4),
                                     scores=np.asarray(p["scores"], np.float32).reshape(-1),
                                     labels=np.asarray(p["labels"], np.int64).reshape(-1)))

    def dets(self, ann: dict) -> List[dict]:
        cat_ids = np.asarray(sorted(int(c["id"]) for c in ann.get("categories", [])), np.int64)
        out = []
        for r in self.results:
            if r["labels"].size and (r["labels"].min() < 0 or r["labels"].max() >= cat_ids.size):
                raise ValueError(f"image {r['img_id']}: label outside the {cat_ids.size} categories of {self.ann_file}")
            out.append(dict(image_id=r["img_id"], bboxes=r["bboxes"], scores=r["scores"],
                            category_ids=cat_ids[r["labels"]]))
        return out

    def write_results(self, dets: List[dict], prefix: str) -> str:
        """``<prefix>.bbox.json`` in COCO results format (mmdet results2json)."""
        recs = []
        for d in dets:
            for b, s, c in zip(d["bboxes"], d["scores"], d["category_ids"]):
                x1, y1, x2, y2 = b.tolist()
                recs.append(dict(image_id=int(d["image_id"]), bbox=[x1, y1, x2 - x1, y2 - y1], score=float(s),
                                 category_id=int(c)))
        path = f"{prefix}.bbox.json"
        d = osp.dirname(path)
        if d:
            os.makedirs(d, exist_ok=True)
        with open(path, "w") as f:
            json.dump(recs, f)
        return path

    def compute_metrics(self, ann: Optional[dict] = None, device="cuda") -> Dict:
        from . import det_eval
        if ann is None:
            if self.ann_file is None:
                raise ValueError(f"{type(self).__name__}: ann_file is required")
            ann = load_annotations(self.ann_file)
        dets = self.dets(ann)
        if self.outfile_prefix is not None:
            self.write_results(dets, self.outfile_prefix)
        if self.format_only:
            return {}
        fn = det_eval.lvis_evaluate if self.lvis else det_eval.coco_evaluate
        ev = fn(ann, dets, classwise=self.classwise, device=device)
        self.eval = ev
        return ev["metrics"]


def _default_iou_thrs():
    from .det_eval import iou_thrs
    return iou_thrs()


@METRICS.register_module()
class CocoMetric(_BoxMetric):
    """mmdet CocoMetric, metric='bbox'."""


@METRICS.register_module()
class LVISMetric(_BoxMetric):
    """mmdet LVISMetric, metric='bbox'."""
    lvis = True


def build_metric(cfg) -> _BoxMetric:
    return METRICS.build(cfg.to_dict() if hasattr(cfg, "to_dict") else dict(cfg))


def metric_lines(ev: dict, lvis: bool) -> List[str]:
    """The summary lines the libraries print: pycocotools ``COCOeval.summarize`` (``iStr``; the first line at
    maxDets 100, see det_eval's docstring) or lvis-api ``LVISEval.print_results``."""
    from .det_eval import COCO_MAX_DETS, LVIS_MAX_DETS, LVIS_STAT_NAMES, iou_thrs
    thrs = iou_thrs()
    all_ious = "{:0.2f}:{:0.2f}".format(thrs[0], thrs[-1])
    if lvis:
        template = " {:<18} {} @[ IoU={:<9} | area={:>6s} | maxDets={:>3d} catIds={:>3s}] = {:0.3f}"
        out = []
        for key, value in zip(LVIS_STAT_NAMES, ev["stats"]):
            title, kind = ("Average Precision", "(AP)") if "AP" in key else ("Average Recall", "(AR)")
            iou = "{:0.2f}".format(float(key[2:]) / 100) if len(key) > 2 and key[2].isdigit() else all_ious
            group = key[2] if len(key) > 2 and key[2] in "rcf" else "all"
            area = key[2] if len(key) > 2 and key[2] in "sml" else "all"
            out.append(template.format(title, kind, iou, area, LVIS_MAX_DETS, group, float(value)))
        return out
    i_str = " {:<18} {} @[ IoU={:<9} | area={:>6s} | maxDets={:>3d} ] = {:0.3f}"
    m0, m1, m2 = COCO_MAX_DETS
    rows = [(1, None, "all", 100), (1, .5, "all", m2), (1, .75, "all", m2), (1, None, "small", m2),
            (1, None, "medium", m2), (1, None, "large", m2), (0, None, "all", m0), (0, None, "all", m1),
            (0, None, "all", m2), (0, None, "small", m2), (0, None, "medium", m2), (0, None, "large", m2)]
    return [i_str.format("Average Precision" if ap == 1 else "Average Recall", "(AP)" if ap == 1 else "(AR)",
                         all_ious if thr is None else "{:0.2f}".format(thr), area, md, float(v))
            for (ap, thr, area, md), v in zip(rows, ev["stats"])]
