"""Test-time augmentation: the pieces of mmcv / mmdet / mmengine that the reference's ``test.py --tta`` block puts together
(test.py:94-127), on this package's path.

    tta_pipeline = [..., WeDetectLetterResize, LoadAnnotations, LoadText,
                    TestTimeAug(transforms=[[RandomFlip(prob=1.), RandomFlip(prob=0.)], [PackDetInputs(meta_keys=...)]])]
    tta_model    = DetTTAModel(module=<the detector>, tta_cfg=dict(nms=dict(type='nms', iou_threshold=0.5), max_per_img=100))

  RandomFlip     mmcv's transform for the two probabilities a TTA pipeline uses: 1 flips the device image through
                 ``wd_flip_u8`` (include/wedetect_hip_views.h), 0 records that it did not
  TestTimeAug    mmcv's transform: one sub-pipeline per element of the Cartesian product of its branch lists
  DetTTAModel    mmdet's wrapper: ``test_step`` takes the views of a batch and hands them to
                 ``YOLOWorldDetector.predict_views`` — one pipelined step per view, ONE merge on the device
                 (``wd_views_merge``: boxes of flipped views mirrored back, mmcv-form batched NMS over the rows of all views),
                 ONE download

``default_tta_cfg`` builds what the reference's block builds when the config has no ``tta_model`` / ``tta_pipeline``, with one
documented deviation: the packed ``meta_keys`` stay the test pipeline's own (``pad_param``, ``texts`` ...) plus
``flip`` and ``flip_direction``.
"""
from __future__ import annotations

import copy
import itertools
from typing import List, Optional, Sequence

import torch

from .registry import MODELS, TRANSFORMS

FLIP_DIRECTIONS = ("horizontal", "vertical", "diagonal")


@TRANSFORMS.register_module()
class RandomFlip:
    """mmcv ``RandomFlip`` as a TTA pipeline uses it: ``prob`` 1 flips ``results['img']`` (device uint8 HWC) and sets
    ``flip=True, flip_direction=direction``; ``prob`` 0 sets ``flip=False, flip_direction=None``.  Nothing else changes:
    ``pad_param`` stays the un-flipped image's, as in the reference (the flip comes after the letter step)."""

    def __init__(self, prob=None, direction: str = "horizontal", **kwargs):
        if kwargs:
            raise NotImplementedError(f"RandomFlip options {sorted(kwargs)} are not on the test path")
        if isinstance(prob, bool) or not isinstance(prob, (int, float)) or float(prob) not in (0.0, 1.0):
            raise NotImplementedError(f"RandomFlip(prob={prob!r}): only prob 0 and 1 (test-time augmentation) are implemented; a "
                                      "random flip is a training transform")
        if direction not in FLIP_DIRECTIONS:
            raise ValueError(f"RandomFlip direction {direction!r}: one of {FLIP_DIRECTIONS}")
        self.prob, self.direction = float(prob), direction

    def __call__(self, results: dict) -> dict:
        if self.prob == 0.0:
            results["flip"], results["flip_direction"] = False, None
            return results
        from . import views as VW
        img = results["img"]
        if not isinstance(img, torch.Tensor) or not img.is_cuda:
            raise RuntimeError("RandomFlip flips on the device: it belongs after LoadImageFromFile / WeDetectLetterResize")
        img = img.contiguous()
        out = torch.empty_like(img)
        VW.flip_u8(img, out, self.direction)
        results["img"] = out
        results["flip"], results["flip_direction"] = True, self.direction
        return results


@TRANSFORMS.register_module()
class TestTimeAug:
    """mmcv ``TestTimeAug``: ``transforms`` is a list of branch lists; every element of their Cartesian product (first list
    outermost) is one sub-pipeline, run on a copy of the input.  Returns ``dict(inputs=[...], data_samples=[...])``, one
    entry per combination (the last transform of a combination packs: ``PackDetInputs``)."""

    __test__ = False                                         # not a pytest class

    def __init__(self, transforms: Sequence[Sequence]):
        from .pipeline import Compose
        if not transforms or any(not isinstance(b, (list, tuple)) or not b for b in transforms):
            raise ValueError("TestTimeAug: transforms must be a non-empty list of non-empty branch lists")
        self.subroutines = [Compose(list(combo)) for combo in itertools.product(*transforms)]

    def __call__(self, results: dict) -> Optional[dict]:
        packed = []
        for sub in self.subroutines:
            r = {k: (v if isinstance(v, torch.Tensor) else copy.deepcopy(v)) for k, v in results.items()}   # tensors are never
            out = sub(r)                                                                                    # written in place
            if out is None:
                return None
            packed.append(out)
        keys = packed[0].keys()
        return {k: [p[k] for p in packed] for k in keys}

    def __repr__(self):
        return "TestTimeAug(" + ", ".join(repr(s) for s in self.subroutines) + ")"


def check_tta_cfg(tta_cfg: Optional[dict]) -> dict:
    """``dict(nms=dict(type='nms', iou_threshold=...[, split_thr]), max_per_img=...)``, validated."""
    from . import views as VW
    cfg = dict(tta_cfg or {})
    if set(cfg) - {"nms", "max_per_img"} or "nms" not in cfg or "max_per_img" not in cfg:
        raise NotImplementedError(f"tta_cfg must hold exactly nms and max_per_img, got {sorted(cfg)}")
    nms = dict(cfg["nms"])
    if nms.get("type", "nms") != "nms":
        raise NotImplementedError(f"tta_cfg.nms.type={nms.get('type')!r}: only the plain greedy 'nms' is implemented")
    if set(nms) - {"type", "iou_threshold", "split_thr"} or "iou_threshold" not in nms:
        raise NotImplementedError(f"tta_cfg.nms must hold type, iou_threshold and optionally split_thr, got {sorted(nms)}")
    iou = float(nms["iou_threshold"])
    if not iou == iou or iou in (float("inf"), float("-inf")):
        raise ValueError("tta_cfg.nms.iou_threshold must be finite")
    m = cfg["max_per_img"]
    if isinstance(m, bool) or int(m) != m or not 1 <= int(m) <= VW.MERGE_MAX_OUT:
        raise NotImplementedError(f"tta_cfg.max_per_img={m!r} outside 1 .. {VW.MERGE_MAX_OUT} (the NMS kernel's kept-list capacity)")
    out = dict(nms=dict(type="nms", iou_threshold=iou), max_per_img=int(m))
    if "split_thr" in nms:
        out["nms"]["split_thr"] = int(nms["split_thr"])
    return out


@MODELS.register_module()
class DetTTAModel:
    """mmdet ``DetTTAModel`` (3.3.0) for box detection: ``merge_preds`` un-flips every view's boxes with
    ``bbox_flip(img_shape=ori_shape)``, concatenates boxes / scores / labels of all views, runs
    ``batched_nms(bboxes, scores, labels, tta_cfg.nms)`` and keeps ``max_per_img`` rows; the result is the FIRST view's
    sample.  Here the whole of it is ``module.predict_views``."""

    def __init__(self, module, tta_cfg: Optional[dict] = None, data_preprocessor=None):
        self.tta_cfg = check_tta_cfg(tta_cfg)
        self.module = MODELS.build(module) if isinstance(module, dict) else module
        if not hasattr(self.module, "predict_views"):
            raise NotImplementedError(f"DetTTAModel: {type(self.module).__name__} has no predict_views (only YOLOWorldDetector does)")

    def __getattr__(self, k):                                # load_state_dict, cuda, set_text_embeddings ... are the module's
        if k in ("module", "tta_cfg"):
            raise AttributeError(k)
        return getattr(self.module, k)

    def cuda(self, device=None):
        self.module.cuda(device)
        return self

    def eval(self):
        self.module.eval()
        return self

    @torch.no_grad()
    def test_step(self, data: dict, stats: Optional[dict] = None) -> List:
        """``data``: mmengine's TTA batch — ``inputs`` a list of V batches ([B, 3, H, W] or lists of [3, H, W]),
        ``data_samples`` a list of V lists of B samples."""
        inputs, samples = data["inputs"], data["data_samples"]
        if not isinstance(inputs, (list, tuple)) or not isinstance(samples, (list, tuple)) or len(inputs) != len(samples) or not inputs:
            raise ValueError("DetTTAModel.test_step: inputs and data_samples must be lists with one entry per view")
        return self.module.predict_views(list(zip(inputs, samples)), self.tta_cfg, stats=stats)


def collate_views(items: Sequence[dict]) -> dict:
    """Pipeline outputs of B images (each ``inputs`` / ``data_samples`` a list of V views) -> the TTA batch: per view the B
    inputs stacked and the B samples listed."""
    n_view = len(items[0]["inputs"])
    if any(len(it["inputs"]) != n_view or len(it["data_samples"]) != n_view for it in items):
        raise ValueError("every image of a batch must have the same number of views")
    return dict(inputs=[torch.stack([it["inputs"][v] for it in items]) for v in range(n_view)],
                data_samples=[[it["data_samples"][v] for it in items] for v in range(n_view)])


DEFAULT_TTA_MODEL = dict(type="DetTTAModel", tta_cfg=dict(nms=dict(type="nms", iou_threshold=0.5), max_per_img=100))


def default_tta_pipeline(test_pipeline: Sequence[dict]) -> list:
    """The reference's default (test.py:103-125): the test pipeline with its last step (PackDetInputs) replaced by the flip
    ``TestTimeAug``.  Deviation: the reference packs ('img_id', 'img_path', 'ori_shape', 'img_shape', 'scale_factor', 'flip',
    'flip_direction') and thereby drops ``pad_param`` (every letterboxed image's boxes are then off by the pad) and ``texts``
    (the class list); here the test pipeline's own ``meta_keys`` are kept and ``flip`` / ``flip_direction`` are added."""
    pipe = copy.deepcopy(list(test_pipeline))
    last = pipe[-1]
    if not isinstance(last, dict) or last.get("type") != "PackDetInputs":
        raise NotImplementedError("the default TTA pipeline replaces a final PackDetInputs; this test pipeline has none")
    from .pipeline import PackDetInputs
    keys = list(last.get("meta_keys", PackDetInputs.DEFAULT_KEYS))
    keys += [k for k in ("flip", "flip_direction") if k not in keys]
    pipe[-1] = dict(type="TestTimeAug",
                    transforms=[[dict(type="RandomFlip", prob=1.0), dict(type="RandomFlip", prob=0.0)],
                                [dict(type="PackDetInputs", meta_keys=tuple(keys))]])
    return pipe
