"""Operator surface of the hot path — the classes callers of the reference construct.

Mirrors (names, arguments, return structures, error behaviour):
  * ``SimpleYOLOWorldDetector``  generate_proposal.py:1052-1218 / extract_embedding.py:1088-1262
        model = SimpleYOLOWorldDetector('base', prompt_dim=768, num_prompts=256)
        model.load_state_dict(ckpt, strict=False); model.cuda(); model.eval()
        outputs = model([path_or_PIL, ...])  ->  list of dict(bboxes, embeddings, scores, labels, scales, bias)
  * ``YOLOWorldDetector``        wedetect/models/detectors/yolo_world.py:19-113, built either from the reference's
        config keywords (``MODELS.build(cfg.model)``: mm_neck, num_train_classes, num_test_classes,
        data_preprocessor, backbone, neck, bbox_head, train_cfg, test_cfg) or directly by size name
        model.reparameterize(texts) / model.test_step(dict(inputs=[...], data_samples=[...]))
        -> data samples with ``.pred_instances.{bboxes, scores, labels}`` (infer_wedetect.py:117-131)

Both are ``torch.nn.Module``s without parameters of their own: the weights live in packed device buffers owned by
``ImageTower``; ``load_state_dict`` / ``state_dict`` / ``_load_from_state_dict`` (what mmengine's ``load_checkpoint``
walks) take and return the reference's key layout.  All tensor math is done by libwedetect_hip.so through
``ImageTower``; this file only does host-side bookkeeping.  There is no CPU fallback: running a detector without a HIP
device / the built library raises.
"""
from __future__ import annotations

import math
import os
from collections import OrderedDict
from typing import Callable, Dict, List, Optional, Sequence, Tuple, Union

import numpy as np
import torch

from .arch import EMBED_DIM, all_params, get_arch
from .guarded import Blob, merged_parts, run_steps
from .registry import MODELS

_IMG_SIZE = {"tiny": (640, 640), "base": (640, 640), "large": (1280, 1280), "nano": (128, 128)}
MAX_OUT_ROWS = 1024          # wd_nms_gather keeps its kept-list in LDS (include/wedetect_hip.h)


# ------------------------------------------------------------------------------------------
# checkpoint key handling
# ------------------------------------------------------------------------------------------
def from_uni_keys(sd: Dict[str, object]) -> Dict[str, object]:
    """Inverse of the remap at generate_proposal.py:1236-1254: accepts the pure-torch module
    names (``backbone.stages...``, ``bbox_head.cls_preds.L.{0,1,3,4,6}``) and returns mmdet
    checkpoint names; keys already in mmdet form pass through."""
    out = {}
    slot_map = {"0": ("0", "conv"), "1": ("0", "bn"), "3": ("1", "conv"), "4": ("1", "bn")}
    for k, v in sd.items():
        nk = k
        if k.startswith("backbone.") and not k.startswith("backbone.image_model.") and not k.startswith("backbone.text_model."):
            nk = "backbone.image_model.model." + k[len("backbone."):]
        elif k.startswith("bbox_head.") and not k.startswith("bbox_head.head_module."):
            parts = k.split(".")
            if parts[1] in ("cls_preds", "reg_preds"):
                slot = parts[3]
                if slot == "6":
                    parts[3] = "2"
                elif slot in slot_map:
                    parts[3:4] = list(slot_map[slot])
            nk = "bbox_head.head_module." + ".".join(parts[1:])
        out[nk] = v
    return out


def _to_numpy_sd(sd) -> Dict[str, np.ndarray]:
    out = {}
    for k, v in sd.items():
        if isinstance(v, torch.Tensor):
            v = v.detach().cpu().float().numpy()
        out[k] = np.asarray(v)
    return out


class _IncompatibleKeys:
    def __init__(self, missing, unexpected):
        self.missing_keys, self.unexpected_keys = list(missing), list(unexpected)

    def __repr__(self):
        if not self.missing_keys and not self.unexpected_keys:
            return "<All keys matched successfully>"
        return f"_IncompatibleKeys(missing_keys={self.missing_keys}, unexpected_keys={self.unexpected_keys})"


# ------------------------------------------------------------------------------------------
# host-side letterbox (the reference's arithmetic with PIL; the detectors use the device version,
# wedetect_amd/preprocess.py, which is bit-exact with it)
# ------------------------------------------------------------------------------------------
def letterbox(img, new_shape=(640, 640), color=(114, 114, 114)):
    """Keep-ratio resize + centred pad to ``new_shape`` (h, w) like generate_proposal.py:17-82:
    r = min(W'/w, H'/h); new size = round(w*r), round(h*r); bilinear; paste at (dw//2, dh//2);
    returns (PIL image, ratio, (dw/2, dh/2)) — note the float half-pads the reference
    subtracts later (1108-1110) next to the integer paste offset."""
    from PIL import Image
    w, h = img.size
    tw, th = new_shape[1], new_shape[0]
    r = min(tw / w, th / h)
    nw, nh = int(round(w * r)), int(round(h * r))
    resized = img.resize((nw, nh), Image.Resampling.BILINEAR)
    dw, dh = tw - nw, th - nh
    canvas = Image.new("RGB", (tw, th), color)
    canvas.paste(resized, (dw // 2, dh // 2))
    return canvas, r, (dw / 2, dh / 2)


class _TowerHolder:
    """Shared plumbing: weights -> packed device tensors -> one ImageTower per (batch, H, W)."""

    def __init__(self, arch: str, num_prompts: int, max_classes: int, max_out: int, precision: Optional[str] = None,
                 nms_pre: int = 30000):
        if max_out > MAX_OUT_ROWS:
            raise NotImplementedError(f"max_per_img / num_proposals {max_out} > {MAX_OUT_ROWS} (the NMS kernel's kept-list capacity)")
        if nms_pre < 1:
            raise ValueError("nms_pre must be positive")
        self.arch = get_arch(arch)
        self.precision = precision
        self._asked_precision = precision          # what the caller configured: restored when a fallen-back tower returns to fp16x3
        self.num_prompts = num_prompts
        self.max_classes, self.max_out, self.nms_pre = max_classes, max_out, nms_pre
        self._sd: Optional[Dict[str, np.ndarray]] = None
        self._packed = None
        self._towers = {}
        self._graphs = {}
        # batches up to this size replay the step from a captured hipGraph; 0 = always eager.  Default 0 since round 5: with the
        # neck / head issued as a DAG on side streams the eager step is as fast as the replay or faster at every small batch
        # (Tiny batch 1: 3.93 ms eager against 4.35 replayed, Base batch 1: 8.18 against 8.25 — profiles/r05_small_batch.txt; the
        # replay was worth 6.6 -> 5.4 ms in round 2, before the step's launch count and host cost came down)
        self.graph_max_batch = int(os.environ.get("WEDETECT_GRAPH_MAX_BATCH", "0"))
        # fp16x3 split scales are chosen from the first batch a tower sees (engine.ImageTower.calibrate); "0": never
        self.auto_calibrate = os.environ.get("WEDETECT_CALIBRATE", "1") != "0"
        # ONE set of split scales per checkpoint, shared by every (B, H, W) tower: an image gets the same bits whatever batch
        # shape it arrives in (per-tower first-batch calibration broke that for checkpoints with scales != 1)
        self.sscale = None
        self.device = None

    def load(self, sd, strict: bool):
        sd = _to_numpy_sd(from_uni_keys(sd))
        want = {name: shape for name, shape, _ in all_params(self.arch, self.num_prompts)}
        missing = [k for k in want if k not in sd]
        unexpected = [k for k in sd if k not in want and not k.endswith("num_batches_tracked")
                      and not k.startswith("backbone.text_model.")
                      and not k.startswith(("backbone.image_model.model.norm.", "backbone.image_model.model.head."))]
        for k, shape in want.items():
            if k in sd and tuple(sd[k].shape) != tuple(shape):
                raise RuntimeError(f"size mismatch for {k}: checkpoint {tuple(sd[k].shape)} vs model {tuple(shape)}")
        if strict and (missing or unexpected):
            raise RuntimeError(f"Error(s) in loading state_dict: missing {missing[:5]}..., unexpected {unexpected[:5]}...")
        if missing:
            raise RuntimeError(f"cannot run with missing tensors (no random-init fallback): {missing[:8]} ...")
        self._sd = {k: sd[k] for k in want}
        self._packed = None
        self._towers.clear()
        self._graphs.clear()
        self.sscale = None                                   # a new checkpoint calibrates anew
        return _IncompatibleKeys(missing, unexpected)

    def state(self) -> "OrderedDict[str, torch.Tensor]":
        return OrderedDict((k, torch.from_numpy(np.array(v))) for k, v in (self._sd or {}).items())

    def tower(self, batch: int, height: int, width: int):
        from .engine import ImageTower
        from .pack import pack
        if self._sd is None:
            raise RuntimeError("load_state_dict() must be called before inference")
        if self.device is None:
            raise RuntimeError("model is not on a HIP device: call .cuda() (there is no CPU execution path)")
        if self._packed is None:
            self._packed = pack(self._sd, self.arch, self.device)
        key = (batch, height, width)
        if key not in self._towers:
            if len(self._towers) >= 4:                       # each tower owns its activation buffers
                old = self._towers.pop(next(iter(self._towers)))
                self._graphs = {k: g for k, g in self._graphs.items() if g.tower is not old}
            self._towers[key] = ImageTower(self.arch, self._packed, batch, height, width, device=self.device,
                                           max_classes=self.max_classes, max_out=self.max_out, nms_pre=self.nms_pre,
                                           precision=self.precision)
            if self.sscale is not None:
                self._towers[key].adopt_scales(self.sscale)
        return self._towers[key]

    def _share_scales(self, tower) -> None:
        self.sscale = dict(tower.sscale)
        for t in self._towers.values():
            if t is not tower:
                t.adopt_scales(self.sscale)

    def recalibrate(self, tower, images_u8) -> None:
        """The range guard tripped under scales taken from an earlier batch: derive them again from this one (scales only go
        down) and hand them to every tower of the checkpoint."""
        tower.calibrate(images_u8, merge=True)
        self._share_scales(tower)

    def calibrate_first(self, tower, images_u8) -> None:
        """Before the first step of a tower (in line or streamed alike).  First batch of this CHECKPOINT: one fp32 pass
        chooses the fp16x3 split scales for its activation ranges (engine.ImageTower.calibrate; scale 1 everywhere for
        ordinary checkpoints); towers of other shapes adopt them."""
        if not tower.calibrated and self.auto_calibrate:
            if self.sscale is None:
                tower.calibrate(images_u8)
                self._share_scales(tower)
            else:
                tower.adopt_scales(self.sscale)

    def detect(self, tower, images_u8, text, meta, text_counts=None, **kw):
        """``tower.detect`` for the detector classes.  Small batches (the reference runs batch 1 everywhere) are
        launch-bound, so the step is replayed from a hipGraph captured on first use (engine.GraphedDetect: inputs are
        copied into the graph's static buffers, results are the tower's usual buffers — bit-identical to the eager
        step, tests/test_gpu_detector.py).  A graph belongs to one (tower, arithmetic mode, bank size, thresholds); the
        range guard's switch to fp32 therefore captures anew."""
        self.calibrate_first(tower, images_u8)
        if kw.get("best_class") or kw.get("sparse_scores") or kw.get("prompt_groups") is not None:
            # single-label, sparse-score and prompt-group steps run eagerly on the unfolded head (the best_scores / sparse_candidates /
            # group_scores sinks of engine.ImageTower._score_bank): no graph, no fold
            return tower.detect(images_u8, text, meta, text_counts=text_counts, **kw)
        if text.dim() == 3 or text_counts is not None:
            # one bank per image ([B, k_max, 768] + device counts): always the eager step, never captured — a graph would
            # have to own a static copy of every packed bank, and a batch of per-image banks is not launch-bound
            return tower.detect(images_u8, text, meta, text_counts=text_counts, **kw)
        if tower.B > self.graph_max_batch:
            return tower.detect(images_u8, text, meta, **kw)
        k = int(text.shape[0])
        if k > tower.max_classes or k > tower.text_norm.shape[0]:
            # a larger bank re-allocates the tower's similarity / top-k buffers: do it BEFORE any capture or replay, and
            # drop every graph of this tower that still points at the old ones (a K=80 graph replayed after a
            # K=100 call would write into freed memory)
            tower._alloc_post(max(k, tower.max_classes))
            if k > tower.text_norm.shape[0]:
                tower.text_norm = torch.empty(k, tower.text_norm.shape[1], dtype=torch.float32, device=tower.dev)
                tower.generation += 1
        self._graphs = {kk: g for kk, g in self._graphs.items() if g.tower is not tower or g.generation == tower.generation}
        key = (id(tower), tower.generation, tower.precision, tower.neck_pin, k, tuple(sorted((a, str(b)) for a, b in kw.items())))
        g = self._graphs.get(key)
        if g is None:
            from .engine import GraphedDetect
            if len(self._graphs) >= 8:
                self._graphs.pop(next(iter(self._graphs)))
            g = self._graphs[key] = GraphedDetect(tower, k, **kw)
            if g.generation != tower.generation:             # cannot happen after the pre-growth above; never replay a stale graph
                raise RuntimeError("tower buffers were re-allocated during graph capture")
        return g(images_u8, text, meta)

    def checked_step(self, tower, images_u8, text, meta, text_counts=None, **kw):
        """The in-line step: ``detect``, then the step's counts through ``ImageTower.checked_counts`` — one D2H sync per
        batch and the fp16x3 range guard, which may recalibrate, repeat the step or fall back to fp32 — then the holder's
        precision follows the tower.  Returns (the tower's result buffers, counts list)."""
        return self.checked_run(tower, images_u8, lambda: self.detect(tower, images_u8, text, meta, text_counts=text_counts, **kw))

    def checked_run(self, tower, images_u8, run):
        """``run()`` (a closure that issues one tower step on ``images_u8`` and returns a result with ``count``) under the range
        guard of ``checked_step``: the guard may recalibrate, repeat ``run`` or fall back to fp32."""
        res = run()
        recal = (lambda: self.recalibrate(tower, images_u8)) if self.auto_calibrate else None
        counts = tower.checked_counts(res, run, recal)
        # towers built later for other shapes start in fp32 too while this one is in its fallback (round 6: not for good — after
        # ImageTower.FALLBACK_RETRY clean batches it re-calibrates and returns to fp16x3, and so does the holder's default)
        self.precision = "fp32" if tower.overflowed else self._asked_precision
        return res, counts

    def inline_only(self) -> bool:
        """True while a tower is in its fp32 fallback: every step then goes in line (wedetect_amd/guarded.py)."""
        return any(t.overflowed for t in self._towers.values())


class _DeviceModule(torch.nn.Module):
    """nn.Module plumbing shared by the two detectors: no parameters, weights in ``self._h`` (a _TowerHolder)."""

    _h: _TowerHolder

    def cuda(self, device=None):
        if not torch.cuda.is_available():
            raise RuntimeError("no HIP device visible: wedetect_amd has no CPU execution path")
        if isinstance(device, (str, torch.device)):
            device = torch.device(device).index
        self._h.device = torch.device("cuda", torch.cuda.current_device() if device is None else device)
        self._on_device(self._h.device)
        return self

    def _on_device(self, device) -> None:
        pass

    def to(self, *args, **kwargs):
        device, dtype, _, _ = torch._C._nn._parse_to(*args, **kwargs)
        if dtype is not None and dtype != torch.float32:
            raise NotImplementedError("the device path computes in fp32 / fp16x3 (ImageTower precision=...); "
                                      f"casting the module to {dtype} is not supported")
        if device is not None:
            if device.type != "cuda":
                raise RuntimeError(f"cannot move to {device}: wedetect_amd has no CPU execution path")
            return self.cuda(device)
        return self

    def half(self):
        return self.to(torch.float16)

    def bfloat16(self):
        return self.to(torch.bfloat16)

    def cpu(self):
        raise RuntimeError("wedetect_amd has no CPU execution path")

    def state_dict(self, *args, destination=None, prefix="", keep_vars=False):
        out = OrderedDict() if destination is None else destination
        for k, v in self._h.state().items():
            out[prefix + k] = v
        return out

    def _load_state(self, state_dict, strict: bool):
        return self._h.load(state_dict, strict)

    def load_state_dict(self, state_dict, strict: bool = True, assign: bool = False):
        if "state_dict" in state_dict and isinstance(state_dict["state_dict"], dict):
            state_dict = state_dict["state_dict"]           # mmengine checkpoint wrapper
        return self._load_state(state_dict, strict)

    def _load_from_state_dict(self, state_dict, prefix, local_metadata, strict, missing_keys, unexpected_keys, error_msgs):
        """The hook torch's and mmengine's recursive loaders call per module: this module takes every key under
        its prefix (there are no child modules holding parameters)."""
        sub = {k[len(prefix):]: v for k, v in state_dict.items() if k.startswith(prefix)}
        try:
            msg = self._load_state(sub, False)
        except RuntimeError as e:
            error_msgs.append(str(e))
            return
        missing_keys.extend(prefix + k for k in msg.missing_keys)
        if strict:
            unexpected_keys.extend(prefix + k for k in msg.unexpected_keys)


# ------------------------------------------------------------------------------------------
# WeDetect-Uni: proposals + embeddings
# ------------------------------------------------------------------------------------------
class SimpleYOLOWorldDetector(_DeviceModule):
    """Drop-in for generate_proposal.py:1052 / extract_embedding.py:1088."""

    def __init__(self, backbone_size, prompt_dim=768, num_prompts=512, num_proposals=300, img_size=None,
                 precision: Optional[str] = None):
        super().__init__()
        if prompt_dim != EMBED_DIM:
            raise ValueError("prompt_dim must be 768")
        self.backbone_size = backbone_size
        self.num_proposals = num_proposals
        self.img_size = tuple(img_size) if img_size is not None else _IMG_SIZE[backbone_size]
        self._h = _TowerHolder(backbone_size, num_prompts, max(num_prompts, 1), num_proposals, precision)
        self._lb = None
        from .lib import TV_TRICK_MAX_NUMEL
        # which execution of the reference the torchvision NMS reproduces: "cpu" (default — the CPU path BASELINE.json's
        # parity contract names: coordinate trick up to 4000 box coordinates, IoU compared with a C++ double threshold) or
        # "cuda" (what the script's hard-coded .cuda() run takes: 20000, float threshold)
        self.tv_nms_device = os.environ.get("WEDETECT_TV_NMS_DEVICE", "cpu")
        if self.tv_nms_device not in TV_TRICK_MAX_NUMEL:
            raise ValueError(f"WEDETECT_TV_NMS_DEVICE must be one of {sorted(TV_TRICK_MAX_NUMEL)}, not {self.tv_nms_device!r}")
        self.tv_trick_max_numel = TV_TRICK_MAX_NUMEL[self.tv_nms_device]

    @torch.no_grad()
    def forward(self, image_paths: Sequence[Union[str, object]], rescale=True) -> List[Dict[str, torch.Tensor]]:
        res, counts, tower = self.forward_batch(image_paths, rescale)
        out = []
        ls = torch.tensor(tower.lvl_logit_scale, dtype=torch.float32, device=self._h.device)
        cb = torch.tensor(tower.lvl_bias, dtype=torch.float32, device=self._h.device)
        for i, n in enumerate(counts):
            lvl = tower.level_of(res["anchors"][i, :n])
            out.append({
                "bboxes": res["bboxes"][i, :n].clone(),
                "embeddings": res["embeddings"][i, :n].clone(),
                "scores": res["scores"][i, :n].clone(),
                "labels": res["labels"][i, :n].to(torch.int64),
                "scales": ls[lvl],
                "bias": cb[lvl],
            })
        return out

    @torch.no_grad()
    def forward_batch(self, image_paths: Sequence[Union[str, object]], rescale=True):
        """The same step with the results left in the tower's fixed-shape device buffers ([B, R, ...] + counts):
        what the multi-GPU gather exchanges (parallel.gather_results).  Returns (buffers, counts list, tower)."""
        from PIL import Image
        from .preprocess import DeviceLetterbox
        if self._h.device is None:
            raise RuntimeError("model is not on a HIP device: call .cuda() (there is no CPU execution path)")
        imgs, metas = [], []
        for p in image_paths:
            imgs.append(Image.open(p).convert("RGB") if isinstance(p, str) else p)
        # letterbox on the device (wd_letterbox_u8, bit-exact with the PIL resize + paste of the
        # reference): the host only decodes and uploads
        if self._lb is None:
            self._lb = DeviceLetterbox(self.img_size, device=self._h.device)
        x, ratios, pads = self._lb(imgs)
        for img, ratio, (dw, dh) in zip(imgs, ratios, pads):
            w, h = img.size if hasattr(img, "size") and not isinstance(img, (np.ndarray, torch.Tensor)) else (img.shape[1], img.shape[0])
            sc = ratio if rescale else 1.0
            metas.append([dw, dh, 0.0, sc, sc, float(w), float(h), 0.0])
        tower = self._h.tower(len(imgs), self.img_size[0], self.img_size[1])
        meta = torch.tensor(metas, dtype=torch.float32, device=self._h.device)
        # torchvision.ops.batched_nms(bbox, scores, labels, 0.7)[:num_proposals] (generate_proposal.py:1210), with the
        # branch threshold of the device the reference's tensors would live on ($WEDETECT_TV_NMS_DEVICE: "cpu" = the CPU
        # reference path the parity contract names, "cuda" = what the script's hard-coded .cuda() run takes)
        res, counts = self._h.checked_step(tower, x, tower.P["prompts"], meta, normalize_text=False, score_thr=0.0, with_embed=True,
                                           nms="torchvision", nms_param=self.tv_trick_max_numel, nms_device=self.tv_nms_device)
        return res, counts, tower

    def predict_stream(self, images_or_paths: Sequence[Union[str, object]], batch_size: int, *, rescale: bool = True,
                       with_embeddings: bool = True, decode_workers: Optional[int] = None, stats: Optional[dict] = None):
        """``forward`` over a whole list of images as a stream of batches (wedetect_amd/stream.py): files are decoded by a
        thread pool into pinned memory, a batch is letterboxed by ONE batched launch sequence (``wd_feed_batch_u8``), the
        steps are pipelined and every batch's results come back in one packed copy.  Yields one dict per image, in input
        order — the fields of ``forward`` as HOST tensors (``embeddings`` unless ``with_embeddings=False``).  ``stats``: a
        dict that receives the stream's counters when it ends."""
        from .stream import UniBackend, predict_stream
        return predict_stream(UniBackend(self, rescale, with_embeddings), images_or_paths, batch_size, decode_workers, stats)


# ------------------------------------------------------------------------------------------
# WeDetect: open-vocabulary detection against a text bank
# ------------------------------------------------------------------------------------------
class InstanceData:
    """Stand-in for mmengine.structures.InstanceData as the reference's scripts and mmdet's result handling use
    it: attribute and item access, boolean-mask / index / slice ``__getitem__``, ``len``, ``keys/values/items``,
    ``cpu / cuda / to / detach / numpy``, ``in``."""

    def __init__(self, metainfo: Optional[dict] = None, **fields):
        object.__setattr__(self, "_f", dict(fields))
        object.__setattr__(self, "_meta", dict(metainfo or {}))

    def __getattr__(self, k):
        try:
            return self._f[k]
        except KeyError:
            if k in self._meta:
                return self._meta[k]
            raise AttributeError(f"InstanceData has no field {k!r}") from None

    def __setattr__(self, k, v):
        if self._f and hasattr(v, "__len__") and len(v) != len(self):
            raise AssertionError(f"the length of values {len(v)} is not consistent with the length of this InstanceData {len(self)}")
        self._f[k] = v

    def __delattr__(self, k):
        del self._f[k]

    def __getitem__(self, item):
        if isinstance(item, str):
            return self._f[item]
        if isinstance(item, int):
            if item >= len(self) or item < -len(self):
                raise IndexError(f"index {item} out of range")
            item = slice(item, None, len(self)) if item >= 0 else slice(item + len(self), None, len(self))
        return InstanceData(self._meta, **{k: (v[item] if not isinstance(v, list) else _index_list(v, item)) for k, v in self._f.items()})

    def __contains__(self, k):
        return k in self._f or k in self._meta

    def __len__(self):
        return len(next(iter(self._f.values()))) if self._f else 0

    def __repr__(self):
        return "<InstanceData(" + ", ".join(f"{k}: {tuple(v.shape) if hasattr(v, 'shape') else type(v).__name__}" for k, v in self._f.items()) + ")>"

    def keys(self):
        return list(self._f.keys())

    def values(self):
        return list(self._f.values())

    def items(self):
        return list(self._f.items())

    def get(self, k, default=None):
        return self._f.get(k, default)

    def _map(self, fn):
        return InstanceData(self._meta, **{k: (fn(v) if isinstance(v, torch.Tensor) else v) for k, v in self._f.items()})

    def cpu(self):
        return self._map(lambda t: t.cpu())

    def cuda(self):
        return self._map(lambda t: t.cuda())

    def to(self, *a, **kw):
        return self._map(lambda t: t.to(*a, **kw))

    def detach(self):
        return self._map(lambda t: t.detach())

    def numpy(self):
        return InstanceData(self._meta, **{k: (v.detach().cpu().numpy() if isinstance(v, torch.Tensor) else v) for k, v in self._f.items()})


def _index_list(v: list, item):
    if isinstance(item, slice):
        return v[item]
    idx = item.tolist() if hasattr(item, "tolist") else list(item)
    if idx and isinstance(idx[0], bool):
        return [x for x, m in zip(v, idx) if m]
    return [v[i] for i in idx]


class DetDataSample:
    """Data sample as ``PackDetInputs`` builds it: ``metainfo`` (also readable as attributes: ``sample.texts``,
    ``sample.ori_shape``, ...) + ``pred_instances`` / ``gt_instances``."""

    def __init__(self, metainfo: Optional[dict] = None, **kw):
        object.__setattr__(self, "_meta", dict(metainfo or {}))
        object.__setattr__(self, "_data", {})
        self._meta.update(kw)

    @property
    def metainfo(self) -> dict:
        return self._meta

    def set_metainfo(self, metainfo: dict) -> None:
        self._meta.update(metainfo)

    def metainfo_keys(self):
        return list(self._meta.keys())

    def keys(self):
        return list(self._data.keys())

    def __contains__(self, k):
        return k in self._data or k in self._meta

    def get(self, k, default=None):
        return self._data.get(k, self._meta.get(k, default))

    def __getattr__(self, k):
        if k in self._data:
            return self._data[k]
        if k in self._meta:
            return self._meta[k]
        if k in ("pred_instances", "gt_instances", "ignored_instances"):
            return None
        raise AttributeError(f"DetDataSample has no attribute {k!r}")

    def __setattr__(self, k, v):
        self._data[k] = v

    def _map(self, name, *a, **kw):
        out = DetDataSample(self._meta)
        for k, v in self._data.items():
            out._data[k] = getattr(v, name)(*a, **kw) if hasattr(v, name) else v
        return out

    def cpu(self):
        return self._map("cpu")

    def cuda(self):
        return self._map("cuda")

    def to(self, *a, **kw):
        return self._map("to", *a, **kw)

    def numpy(self):
        return self._map("numpy")


def _meta_of(sample) -> dict:
    if sample is None:
        return {}
    if isinstance(sample, dict):
        return sample.get("metainfo", sample)
    return getattr(sample, "metainfo", {}) or {}


def _as_sample(sample) -> DetDataSample:
    """``None`` / a dict (its ``metainfo``) / a data sample -> the data sample that takes the predictions."""
    if sample is None:
        return DetDataSample()
    return DetDataSample(metainfo=_meta_of(sample)) if isinstance(sample, dict) else sample


def _batch_hw(xs: Sequence[torch.Tensor], what: str = "") -> Tuple[int, int]:
    """(H, W) of a batch of [3, H, W] inputs of one shape, H and W multiples of 32; ``what`` prefixes the error texts."""
    shapes = {tuple(t.shape) for t in xs}
    if len(shapes) != 1 or len(next(iter(shapes))) != 3 or next(iter(shapes))[0] != 3:
        raise ValueError(f"{what}inputs must be [3, H, W] tensors of one shape after the test pipeline, got {sorted(shapes)}")
    _, hh, ww = next(iter(shapes))
    if hh % 32 or ww % 32:
        raise ValueError(f"{what}input size {hh}x{ww} is not a multiple of 32 (letterbox to img_scale first)")
    return int(hh), int(ww)


def _nhwc_u8(xs: Sequence[torch.Tensor], dev, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """A checked batch (``_batch_hw``) of BGR [3, H, W] inputs -> the tower's RGB NHWC uint8 batch on ``dev``, written into
    ``out`` when given: bgr_to_rgb + NHWC (data_preprocessor.py:35-36)."""
    from . import lib as L
    chw = torch.stack([x.to(dev) for x in xs])               # [b, 3, H, W] BGR, contiguous
    if chw.dtype not in (torch.uint8, torch.float32):
        chw = chw.to(torch.float32)
    if out is None:
        out = torch.empty(chw.shape[0], chw.shape[2], chw.shape[3], 3, dtype=torch.uint8, device=dev)
    L.chw_to_hwc_u8(chw, out)
    return out


def _tiled_ctl_parts(total: int) -> tuple:
    """The control block of ``predict_tiled`` (guarded.layout): the tile descriptors, then the per-tile metadata."""
    from .tiling import TILE_DTYPE
    return (("plan", (total * TILE_DTYPE.itemsize,), torch.uint8), ("meta", (total, 8), torch.float32))


def _views_ctl_parts(V: int, B: int) -> tuple:
    """The control block of ``predict_views`` (guarded.layout): flip codes, image sizes, per-view metadata."""
    return (("flip", (V,), torch.int32), ("wh", (B, 2), torch.float32), ("meta", (V, B, 8), torch.float32))


def _flat_texts(texts) -> Tuple[str, ...]:
    """``[[a], [b]]`` (reparameterize, infer_wedetect.py:165-167), ``[a, b]`` (what LoadText leaves in a data sample,
    mm_transforms.py:126-133) -> ``(a, b)``: one caption per class, the first of each list."""
    return tuple((t[0] if isinstance(t, (list, tuple)) else t) for t in texts)


# Per-image banks are packed to [b, k_max, 768] with k_max rounded UP to a multiple of this.  The tower sizes its score,
# top-k and normalised-bank buffers by the largest k_max it has seen and re-allocates (dropping captured graphs) whenever
# a larger one arrives: with the rounding a stream of batches whose longest class list wanders (37, 41, 44 ...) settles after
# a few sizes instead of re-allocating at every new maximum.  16 keeps the padding the top-k has to read below 16 columns
# (none at the usual 80), and a multiple of 4 keeps every score row 16-byte aligned for the kernel's vector stores.
BANK_K_ROUND = 16


def round_bank_k(k: int) -> int:
    """k_max of a packed bank for a longest class list of ``k`` rows."""
    if k < 1:
        raise ValueError("a class bank needs at least one row")
    return -(-int(k) // BANK_K_ROUND) * BANK_K_ROUND


def bank_pack_key(banks: Sequence[torch.Tensor]) -> Optional[Tuple[int, ...]]:
    """Cache key of a batch's banks: None when every sample carries the SAME bank object (the shared-bank step), else the
    identities of the bank objects in sample order (a cache entry keeps the objects alive, so an id cannot be recycled
    while its entry exists)."""
    if not banks:
        raise ValueError("no banks")
    if all(b is banks[0] for b in banks):
        return None
    return tuple(id(b) for b in banks)


def letterbox_meta(m: dict, hh: int, ww: int, rescale: bool) -> List[float]:
    """The post-process's 8 floats of one image from its sample's metainfo (``pad_param``, ``scale_factor``,
    ``ori_shape``; an [hh, ww] input that was never letterboxed when they are missing)."""
    ori = m.get("ori_shape", (hh, ww))
    sf = m.get("scale_factor", (1.0, 1.0))
    pad = m.get("pad_param", None)
    px, py = (0.0, 0.0) if pad is None else (float(pad[2]), float(pad[0]))
    sx, sy = (float(sf[0]), float(sf[1])) if rescale else (1.0, 1.0)
    if not rescale:
        px = py = 0.0
    return [px, py, 0.0, sx, sy, float(ori[1]), float(ori[0]), 1.0]


def pack_image_banks(banks: Sequence[torch.Tensor], device=None) -> Tuple[torch.Tensor, torch.Tensor]:
    """Banks [k_i, 768] of one batch -> (packed [b, k_max, 768] float32 with zero rows below each bank, counts int32 [b]),
    both on ``device``; k_max = round_bank_k(max k_i).  Rows are copied as they are (the tower normalises on the device)."""
    for b in banks:
        if b.dim() != 2 or b.shape[1] != EMBED_DIM or b.shape[0] < 1:
            raise ValueError(f"a class bank must be [K >= 1, {EMBED_DIM}], got {tuple(b.shape)}")
    ks = [int(b.shape[0]) for b in banks]
    packed = torch.zeros(len(banks), round_bank_k(max(ks)), EMBED_DIM, dtype=torch.float32, device=device)
    for i, b in enumerate(banks):
        packed[i, : ks[i]].copy_(b)
    return packed, torch.tensor(ks, dtype=torch.int32).to(packed.device)


def plan_exemplars(exemplars, names=None, anchors_per_box: int = 4, min_iou: float = 0.1) -> dict:
    """The host side of an exemplar-bank build (include/wedetect_hip_exemplar.h): ``exemplars[b]`` = the list of
    ``(box_xyxy_in_original_pixels, class_index)`` of image b -> ``ex_boxes`` fp32 [B, max_ex, 4], ``ex_count`` int32 [B], the
    classes' slot lists ``cls_off`` int32 [C + 1] / ``cls_slot`` int32 [T] (class by class: images in batch order, an image's
    examples in list order, an example's anchors by rank), ``cls_examples`` (the (b, e) pairs of every class) and ``names``.
    ValueError for a box with non-positive width or height (or a non-finite coordinate), a class index outside 0 .. C - 1, a
    class without an example, more than 64 examples in one image; C = len(names), or the largest index + 1 without names."""
    from . import exemplar as EX
    m, min_iou = EX.check_m(anchors_per_box), EX.check_min_iou(min_iou)
    flat = [(b, e, box, cls) for b, lst in enumerate(exemplars) for e, (box, cls) in enumerate(lst)]
    if not flat:
        raise ValueError("exemplars: no example box in the batch")
    for b, e, box, cls in flat:
        box = [float(v) for v in box]
        if len(box) != 4 or not all(math.isfinite(v) for v in box) or not (box[2] > box[0] and box[3] > box[1]):
            raise ValueError(f"exemplars[{b}][{e}]: box {box} must be (x1, y1, x2, y2) with positive width and height")
        if isinstance(cls, bool) or int(cls) != cls or cls < 0:
            raise ValueError(f"exemplars[{b}][{e}]: class index {cls!r} must be a non-negative int")
    n_cls = len(names) if names is not None else max(int(cls) for *_, cls in flat) + 1
    names = [str(n) for n in names] if names is not None else [f"exemplar_{c}" for c in range(n_cls)]
    max_ex = max(len(lst) for lst in exemplars)
    if max_ex > EX.MAX_EX:
        raise ValueError(f"exemplars: at most {EX.MAX_EX} example boxes per image, got {max_ex}")
    ex_boxes, ex_count = np.zeros((len(exemplars), max_ex, 4), np.float32), np.zeros(len(exemplars), np.int32)
    cls_examples: List[List[Tuple[int, int]]] = [[] for _ in range(n_cls)]
    for b, e, box, cls in flat:
        if int(cls) >= n_cls:
            raise ValueError(f"exemplars[{b}][{e}]: class index {cls} outside the {n_cls} names")
        ex_boxes[b, e] = box
        ex_count[b] = max(ex_count[b], e + 1)
        cls_examples[int(cls)].append((b, e))
    for c, lst in enumerate(cls_examples):
        if not lst:
            raise ValueError(f"class {c} ({names[c]!r}) has no example box")
    s = max_ex * m
    slots = [[b * s + e * m + j for b, e in lst for j in range(m)] for lst in cls_examples]
    cls_off = np.cumsum([0] + [len(v) for v in slots]).astype(np.int32)
    return dict(ex_boxes=ex_boxes, ex_count=ex_count, cls_off=cls_off, cls_slot=np.concatenate(slots).astype(np.int32),
                cls_examples=cls_examples, names=names, m=m, min_iou=min_iou, max_ex=max_ex)


def plan_tune_boxes(boxes, n_rows=None, anchors_per_box: int = 4, min_iou: float = 0.1) -> dict:
    """The host side of a bank-tuning batch (include/wedetect_hip_tune.h): ``boxes[b]`` = the list of
    ``(box_xyxy_in_original_pixels, class_index)`` of image b -> ``ex_boxes`` fp32 [B, max_ex, 4], ``ex_count`` int32 [B],
    ``gt_cls`` int32 [B, max_ex].  The box checks of ``plan_exemplars``; unlike there a class may be without a box (frozen rows,
    classes that learn from negatives only) and an image may be without one (all its anchors are negatives).  ``n_rows``: the rows
    of the bank the class indices refer to, when known."""
    from . import exemplar as EX
    m, min_iou = EX.check_m(anchors_per_box), EX.check_min_iou(min_iou)
    flat = [(b, e, box, cls) for b, lst in enumerate(boxes) for e, (box, cls) in enumerate(lst)]
    for b, e, box, cls in flat:
        box = [float(v) for v in box]
        if len(box) != 4 or not all(math.isfinite(v) for v in box) or not (box[2] > box[0] and box[3] > box[1]):
            raise ValueError(f"boxes[{b}][{e}]: box {box} must be (x1, y1, x2, y2) with positive width and height")
        if isinstance(cls, bool) or int(cls) != cls or cls < 0:
            raise ValueError(f"boxes[{b}][{e}]: class index {cls!r} must be a non-negative int")
        if n_rows is not None and int(cls) >= n_rows:
            raise ValueError(f"boxes[{b}][{e}]: class index {cls} outside the {n_rows} rows of the bank")
    max_ex = max([len(lst) for lst in boxes] + [1])
    if max_ex > EX.MAX_EX:
        raise ValueError(f"boxes: at most {EX.MAX_EX} labelled boxes per image, got {max_ex}")
    ex_boxes, ex_count = np.zeros((len(boxes), max_ex, 4), np.float32), np.zeros(len(boxes), np.int32)
    gt_cls = np.zeros((len(boxes), max_ex), np.int32)
    for b, e, box, cls in flat:
        ex_boxes[b, e], gt_cls[b, e] = box, int(cls)
        ex_count[b] = max(ex_count[b], e + 1)
    return dict(ex_boxes=ex_boxes, ex_count=ex_count, gt_cls=gt_cls, m=m, min_iou=min_iou, max_ex=max_ex)


class MultiModalYOLOBackbone:
    """``model.backbone`` of the reference detector (mm_backbone.py:594-656) as far as inference callers touch it:
    ``forward_text(texts)`` and ``with_text_model``.  The image side is the fused ``ImageTower``; it has no
    per-module forward."""

    def __init__(self, image_model, text_model=None, frozen_stages: int = -1, with_text_model: bool = True, **kw):
        self.image_model = MODELS.build(image_model) if isinstance(image_model, dict) else image_model
        self.text_model = MODELS.build(text_model) if isinstance(text_model, dict) else text_model
        self.with_text_model = self.text_model is not None and with_text_model

    def forward_text(self, text: List[List[str]]) -> torch.Tensor:
        assert self.with_text_model, "forward_text() requires a text model"          # mm_backbone.py:648
        return self.text_model(text)

    def forward_image(self, image):
        raise NotImplementedError("the image tower is one fused launch sequence (engine.ImageTower): use "
                                  "YOLOWorldDetector.predict / test_step")


class YOLOWorldDetector(_DeviceModule):
    """Drop-in for the configured ``YOLOWorldDetector`` (mm_neck=False, use_bn_head=True).

    Two ways to construct it.  (1) The reference's keywords, as ``MODELS.build(cfg.model)`` passes them
    (yolo_world.py:15-24 + the mmdet single-stage detector's ``data_preprocessor, backbone, neck, bbox_head, train_cfg,
    test_cfg``): the dicts are validated by ``config.check_model_cfg`` — unknown registry names raise ``KeyError``,
    options outside the implemented path ``NotImplementedError`` — and the text tower named by
    ``backbone.text_model`` is wired in, so ``reparameterize(texts)`` works as at yolo_world.py:58-61.
    (2) ``YOLOWorldDetector("base", test_cfg=..., text_encoder=...)`` for callers without a config.

    ``test_cfg`` keeps the reference's keys (config/wedetect_base.py:18-25).  Inputs may have any H x W that is a
    multiple of 32 (one ImageTower is kept per shape); ``img_scale`` = (H, W) is only the default shape."""

    def __init__(self, model_size: Optional[str] = None, img_scale=None, test_cfg=None,
                 text_encoder: Optional[Callable] = None, max_classes: Optional[int] = None, precision: Optional[str] = None,
                 *, mm_neck: bool = False, num_train_classes: int = 80, num_test_classes: int = 80,
                 data_preprocessor=None, backbone=None, neck=None, bbox_head=None, train_cfg=None, init_cfg=None,
                 tokenizer=None, best_class: bool = False, agnostic_nms: bool = False, sparse_scores: bool = False,
                 sparse_cap: int = 65536, top_names: int = 0, prompt_groups: bool = False):
        super().__init__()
        # prompt groups (also ``model.prompt_groups`` of a config): every class is scored as the best of ALL its prompts — the
        # synonym lists of the class-text files — instead of its first caption (wedetect_amd/groups.py, engine.ImageTower.detect)
        self.prompt_groups = bool(prompt_groups)
        self._tuner = None                                   # tune_bank's cache between fit=False calls (tune.BankTuner)
        self._tracker = None                                 # track()'s own track.Tracker, made by its first call
        if self.prompt_groups and (best_class or sparse_scores or top_names):
            raise ValueError("prompt_groups=True is a multi-label dense step of its own: it excludes best_class, sparse_scores and top_names")
        self._plans: Dict[Tuple[str, ...], object] = {}      # first captions -> groups.PromptGroups of that bank (prompt_groups only)
        self._plan_cur = None                                # the plan of ``text_feats``
        # the n best names of every detection (also ``model.top_names`` of a config): the best-class step that keeps the
        # near-winners; ``pred_instances`` gains ``top_labels`` / ``top_scores`` [m, n] (engine.ImageTower.detect)
        if isinstance(top_names, bool) or not isinstance(top_names, int) or not 0 <= top_names <= 8:
            raise ValueError(f"top_names must be an int in 0..8, got {top_names!r}")
        if top_names and not best_class:
            raise ValueError("top_names needs best_class=True: it is the single-label step with the near-winners kept")
        self.top_names = top_names
        # sparse scores (also ``model.sparse_scores`` / ``model.sparse_cap`` of a config): the multi-label step whose similarity
        # launch writes candidate lists of ``sparse_cap`` keys per image instead of the [B, N, K] scores (engine.ImageTower.detect)
        self.sparse_scores, self.sparse_cap = bool(sparse_scores), int(sparse_cap)
        if self.sparse_scores and best_class:
            raise ValueError("sparse_scores=True is the multi-label step and best_class=True the single-label one: choose one")
        if self.sparse_scores and not 1 <= self.sparse_cap <= 1 << 20:
            raise ValueError("sparse_cap must lie in 1 .. 2^20 keys per image")
        # single-label detection (the reference's test_cfg.multi_label=False / nms.class_agnostic=True, asked for with keywords
        # of this class — also ``model.best_class`` / ``model.agnostic_nms`` of a config; ``test_cfg`` keeps the reference's keys)
        self.best_class, self.agnostic_nms = bool(best_class), bool(agnostic_nms)
        if self.agnostic_nms and not self.best_class:
            raise NotImplementedError("agnostic_nms=True is built for best_class=True only (one label per region)")
        self.mm_neck, self.num_train_classes, self.num_test_classes = mm_neck, num_train_classes, num_test_classes
        self.backbone: Optional[MultiModalYOLOBackbone] = None
        if backbone is not None:
            from .config import check_model_cfg
            model_cfg = dict(type="YOLOWorldDetector", mm_neck=mm_neck, num_train_classes=num_train_classes,
                             num_test_classes=num_test_classes, data_preprocessor=data_preprocessor, backbone=backbone,
                             neck=neck, bbox_head=bbox_head, train_cfg=train_cfg, test_cfg=test_cfg)
            size = check_model_cfg(model_cfg)
            if model_size is not None and model_size != size:
                raise ValueError(f"model_size={model_size!r} contradicts the config ({size!r})")
            model_size = size
            self.backbone = MultiModalYOLOBackbone(backbone["image_model"], backbone.get("text_model"))
            if self.backbone.text_model is not None:
                if tokenizer is not None:
                    self.backbone.text_model.tokenizer = tokenizer
                if precision is not None:
                    self.backbone.text_model.precision = precision
            if max_classes is None:
                max_classes = max(int(num_test_classes), 1)
        elif model_size is None:
            raise TypeError("YOLOWorldDetector needs either the config keywords (backbone=..., neck=..., bbox_head=...) or a model_size")
        cfg = dict(multi_label=True, nms_pre=30000, score_thr=0.001, nms=dict(type="nms", iou_threshold=0.7),
                   max_per_img=300)
        cfg.update(test_cfg or {})
        if not cfg["multi_label"]:
            raise NotImplementedError("test_cfg.multi_label=False is not read from test_cfg (only multi_label=True, every shipped "
                                      "config); single-label detection is the keyword best_class=True of this class")
        nms = dict(cfg["nms"])
        if nms.get("type", "nms") != "nms":
            raise NotImplementedError(f"test_cfg.nms.type={nms.get('type')!r}: only the plain greedy 'nms' is implemented")
        # mmcv.ops.batched_nms options (mmcv/ops/nms.py 2.1.0).  max_num: ``keep[:max_num]`` after NMS — followed by mmdet's
        # ``results[:max_per_img]``, i.e. min(max_num, max_per_img) rows.  score_threshold: ``scores > score_threshold`` before
        # NMS — the candidates already passed ``scores > score_thr`` and the nms_pre cut keeps the highest, so the two filters are
        # one with the larger threshold.  class_agnostic: NMS on the un-offset boxes across classes — not built.
        if nms.get("class_agnostic", False):
            raise NotImplementedError("test_cfg.nms.class_agnostic=True (mmcv.ops.batched_nms on un-offset boxes across classes) "
                                      "is not read from test_cfg; every shipped config uses class-aware NMS.  With best_class=True the "
                                      "keyword agnostic_nms=True of this class gives that NMS")
        if set(nms) - {"type", "iou_threshold", "split_thr", "class_agnostic", "max_num", "score_threshold"}:
            raise NotImplementedError("test_cfg.nms options "
                                      f"{sorted(set(nms) - {'type', 'iou_threshold', 'split_thr', 'class_agnostic', 'max_num', 'score_threshold'})} are not implemented")
        max_num = int(nms.get("max_num", -1))
        if max_num > 0:
            cfg["max_per_img"] = min(int(cfg["max_per_img"]), max_num)
        if float(nms.get("score_threshold", 0.0)) > float(cfg["score_thr"]):
            # mmcv decides between its one-call and its per-class branch on the candidate count BEFORE this filter
            # (boxes.shape[0] < split_thr, mmcv/ops/nms.py batched_nms), the merged filter decides on the count after it: the two
            # can only differ when nms_pre candidates can reach split_thr — then the option is refused rather than emulated
            # with last-bit IoU differences.  No shipped config sets score_threshold.
            if int(cfg["nms_pre"]) >= int(nms.get("split_thr", 10000)):
                raise NotImplementedError("test_cfg.nms.score_threshold above score_thr with nms_pre >= split_thr: mmcv picks its NMS "
                                          "branch on the pre-filter candidate count, which the merged filter cannot reproduce; raise "
                                          "score_thr instead, or lower nms_pre below split_thr")
            cfg["score_thr"] = float(nms["score_threshold"])
        self.test_cfg = cfg
        self.model_size = model_size
        self.img_scale = tuple(img_scale) if img_scale is not None else _IMG_SIZE[model_size]
        self._h = _TowerHolder(model_size, 0, max_classes if max_classes is not None else 1203, int(cfg["max_per_img"]),
                               precision, nms_pre=int(cfg["nms_pre"]))
        self.text_encoder = text_encoder
        self.texts = None
        self.text_feats: Optional[torch.Tensor] = None
        self._banks: Dict[Tuple[str, ...], torch.Tensor] = {}
        # packed per-image banks of recurring bank combinations: key -> (the bank objects, packed [b, k_max, 768], counts)
        self._packed_banks: "OrderedDict[Tuple[int, ...], tuple]" = OrderedDict()

    # -- weights --------------------------------------------------------------------------
    def _load_state(self, state_dict, strict: bool):
        msg = self._h.load(state_dict, strict)
        tm = self.backbone.text_model if self.backbone is not None else None
        if tm is not None:
            sub = {k: v for k, v in state_dict.items() if k.startswith("backbone.text_model.")}
            if sub:
                tm.load_state_dict(sub)
            elif strict:
                raise RuntimeError("Error(s) in loading state_dict: no backbone.text_model.* tensors in the checkpoint")
        self._banks.clear()
        self._packed_banks.clear()
        self.text_feats = self.texts = None
        return msg

    def state_dict(self, *args, destination=None, prefix="", keep_vars=False):
        out = super().state_dict(destination=destination, prefix=prefix)
        tm = self.backbone.text_model if self.backbone is not None else None
        if tm is not None:
            for k, v in tm.state_dict().items():
                out[prefix + "backbone.text_model." + k] = v
        return out

    def _on_device(self, device) -> None:
        tm = self.backbone.text_model if self.backbone is not None else None
        if tm is not None:
            tm.cuda(device)

    # -- text side ------------------------------------------------------------------------
    def set_text_embeddings(self, feats: torch.Tensor, texts: Optional[List[List[str]]] = None) -> None:
        """Class bank [K, 768] (any norm: it is L2-normalised on device like
        BNContrastiveHead does, yolo_world_head.py:101)."""
        if feats.dim() == 3:
            if feats.shape[0] != 1:
                raise ValueError("a [B, K, 768] bank must have B == 1 (one bank for the whole batch)")
            feats = feats[0]
        if feats.dim() != 2 or feats.shape[1] != EMBED_DIM:
            raise ValueError("text embeddings must be [K, 768]")
        if self.prompt_groups:
            # the bank holds one row per PROMPT, class after class; the tower sees it padded to bins of 32 rows (groups.PromptGroups)
            if texts is None:
                raise ValueError("prompt_groups=True: set_text_embeddings needs the class lists (texts) the [P, 768] rows belong to")
            from .groups import PromptGroups
            plan = PromptGroups.from_texts(texts)
            if feats.shape[0] != plan.P:
                raise ValueError(f"prompt_groups=True: text embeddings must be ({plan.P}, {EMBED_DIM}), one row per prompt of the "
                                 f"{plan.G} classes, got {tuple(feats.shape)}")
            feats = plan.pad_bank(feats.detach().to(torch.float32))
            self._plans[_flat_texts(texts)] = self._plan_cur = plan
        self.text_feats = feats.detach().to(torch.float32)
        self.texts = texts
        if texts is not None:
            self._banks[_flat_texts(texts)] = self.text_feats

    def _encode(self, flat: Tuple[str, ...]) -> torch.Tensor:
        if self.backbone is not None and self.backbone.with_text_model:
            return self.backbone.forward_text([list(flat)])[0]              # [1, K, D] -> [K, D]
        if self.text_encoder is not None:
            return self.text_encoder(list(flat))
        raise NotImplementedError("no text tower: build the detector from a config with backbone.text_model, pass "
                                  "text_encoder=..., or call set_text_embeddings(bank)")

    def reparameterize(self, texts: List[List[str]]) -> None:
        """yolo_world.py:58-61: ``self.texts = texts; self.text_feats = self.backbone.forward_text(texts)``."""
        flat = _flat_texts(texts)
        if self.prompt_groups:                               # ALL prompts of every class, class after class
            flat = tuple(p for t in texts for p in ([t] if isinstance(t, str) else t))
        self.set_text_embeddings(self._encode(flat), texts)

    def _bank_for(self, sample) -> torch.Tensor:
        """extract_feat (yolo_world.py:82-113): data samples that carry ``texts`` are scored against those texts; the
        reference re-runs the text tower for every image, here the bank of each distinct class list is built once."""
        texts = _meta_of(sample).get("texts") if sample is not None else None
        if texts is None:
            if self.text_feats is None:
                raise RuntimeError("no class bank: call reparameterize(texts) or set_text_embeddings(bank) first, or "
                                   "pack `texts` into the data samples")
            return self.text_feats
        flat = _flat_texts(texts)
        bank = self._banks.get(flat)
        if bank is None:
            if len(self._banks) > 64:
                self._banks.clear()
                self._plans.clear()
            if self.prompt_groups:
                # a class list seen for the first time in a data sample: grouped as it is given (LoadText leaves first captions
                # only — classes of one prompt; banks with synonyms come through reparameterize / set_text_embeddings)
                from .groups import PromptGroups
                plan = self._plans[flat] = PromptGroups.from_texts(texts)
                bank = self._banks[flat] = plan.pad_bank(self._encode(tuple(plan.flat)).detach().to(torch.float32))
                return bank
            bank = self._banks[flat] = self._encode(flat).detach().to(torch.float32)
        return bank

    def _plan_for(self, sample):
        """The packing plan of the bank ``_bank_for(sample)`` returns (prompt_groups only)."""
        texts = _meta_of(sample).get("texts") if sample is not None else None
        return self._plan_cur if texts is None else self._plans[_flat_texts(texts)]

    PACKED_BANKS_MAX = 16          # cached combinations (32 banks of 80 rows: 7.9 MB each)

    def _packed_for(self, banks: List[torch.Tensor], dev):
        """None when the whole batch shares one bank object; else the packed banks and device counts of this combination,
        built once (pack_image_banks) and kept while the combination recurs."""
        key = bank_pack_key(banks)
        if key is None:
            return None
        hit = self._packed_banks.get(key)
        if hit is not None and hit[1].device == dev and all(a is b for a, b in zip(hit[0], banks)):
            self._packed_banks.move_to_end(key)
            return hit[1], hit[2]
        while len(self._packed_banks) >= self.PACKED_BANKS_MAX:
            self._packed_banks.popitem(last=False)
        packed, counts = pack_image_banks(banks, dev)
        self._packed_banks[key] = (tuple(banks), packed, counts)
        return packed, counts

    # -- image side -----------------------------------------------------------------------
    @torch.no_grad()
    def test_step(self, data: dict):
        inputs, samples = data["inputs"], data.get("data_samples")
        if samples is None:
            samples = [None] * len(inputs)
        return self.predict(inputs, samples)

    def forward(self, inputs, data_samples=None, mode: str = "predict"):
        if mode != "predict":
            raise NotImplementedError(f"mode={mode!r}: only inference ('predict') is on this path")
        return self.predict(inputs, data_samples if data_samples is not None else [None] * len(inputs))

    @torch.no_grad()
    def predict(self, batch_inputs, batch_data_samples, rescale: bool = True):
        """batch_inputs: list / tensor of [3, H, W] images as the mmdet pipeline packs them
        (uint8 or float 0-255, BGR — DetDataPreprocessor does bgr_to_rgb and /255,
        wedetect_base.py:44-48), all of one shape with H, W multiples of 32 (the test pipeline letterboxes
        to ``img_scale``)."""
        res, counts, samples = self._predict_step(batch_inputs, batch_data_samples, rescale)
        return self._instances(res, counts, samples)

    def _predict_step(self, batch_inputs, batch_data_samples, rescale: bool, **over):
        """The guarded tower step of ``predict`` (``over``: keywords that replace the step's own, e.g. ``with_embed``).  Returns
        (the tower's result buffers, the counts on the host, the samples as a list)."""
        dev = self._h.device
        if dev is None:
            raise RuntimeError("model is not on a HIP device: call .cuda()")
        xs = [x for x in batch_inputs]
        samples = list(batch_data_samples) if batch_data_samples is not None else [None] * len(xs)
        if len(samples) != len(xs):
            raise ValueError(f"{len(xs)} inputs but {len(samples)} data samples")
        banks = [self._bank_for(s) for s in samples]
        hh, ww = _batch_hw(xs)
        # ONE tower step for the batch, whatever the samples' class lists: one bank object for all -> the shared-bank step;
        # otherwise the banks travel as [b, k_max, 768] + device counts and every image is scored against its own
        # (yolo_world.py:94-96: ``texts = [data_sample.texts for data_sample in batch_data_samples]``)
        packed = self._packed_for(banks, dev)
        kw = self._step_kw(modes=True)
        if self.prompt_groups:
            if packed is not None:
                raise NotImplementedError("prompt_groups=True with differing class lists in one batch is not implemented (one "
                                          "packing plan per step); batch images of one class list")
            kw["prompt_groups"] = self._plan_for(samples[0])
        x = _nhwc_u8(xs, dev)
        tower = self._h.tower(len(xs), hh, ww)
        meta = torch.tensor([letterbox_meta(_meta_of(s), hh, ww, rescale) for s in samples], dtype=torch.float32, device=dev)
        bank, counts_dev = (banks[0].to(dev), None) if packed is None else packed
        kw.update(over)
        res, counts = self._h.checked_step(tower, x, bank, meta, text_counts=counts_dev, **kw)
        return res, counts, samples

    def _instances(self, res, counts, samples, extra=()):
        """``pred_instances`` of every sample from a step's result buffers; ``extra``: (field, [B, max_out] tensor) pairs that are
        cut to the counts like the others."""
        out = []
        for j, n in enumerate(counts):
            inst = InstanceData(bboxes=res["bboxes"][j, :n].clone(), scores=res["scores"][j, :n].clone(),
                                labels=res["labels"][j, :n].to(torch.int64))
            if self.top_names:
                inst.top_labels = res["top_labels"][j, :n].to(torch.int64)
                inst.top_scores = res["top_scores"][j, :n].clone()
            for name, t in extra:
                setattr(inst, name, t[j, :n].clone())
            s = _as_sample(samples[j])
            s.pred_instances = inst
            out.append(s)
        return out

    # -- tracking ----------------------------------------------------------------------------
    @torch.no_grad()
    def track(self, batch_inputs, batch_data_samples, rescale: bool = True, n_seq: int = 1, tracker=None, track_params=None,
              assignment=None):
        """``predict`` for the frames of a video, plus persistent ids: ``pred_instances`` gains ``track_ids`` (int32, 0 = the
        detection belongs to no track) and ``track_hits`` (frames the track was matched in), on the device like the other fields.
        The batch holds ``n_seq`` independent sequences of ``len(batch) / n_seq`` consecutive frames each, image s * n_frame + f
        being frame f of sequence s: one video -> ``n_seq=1``, one frame of each of B cameras -> ``n_seq=B``.  The tracks live in
        ``tracker`` (a ``track.Tracker``; the detector makes and keeps one, with ``track_params`` — a ``track.TrackParams`` — on
        the first call) and carry over from call to call; ``reset_tracks()`` clears them.  ``assignment`` ("greedy", the default,
        or "optimal": the maximum-weight matching of include/addons/wedetect_hip_assign.h in place of the greedy picks) goes to the
        tracker the detector makes and must not differ from the kept one's; with a ``tracker`` passed in it must be None.

        The association (include/wedetect_hip_track.h: two greedy rounds on IoU and the kept rows' region embeddings) is ONE
        launch behind the tower step, with no host synchronisation of its own: the step runs with ``with_embed=True`` under the
        range guard of ``predict``, and the tracker is launched only after the guard has settled the step, so a step that is
        repeated never reaches the tracks.  Every field ``predict`` fills has the same bits.

        Works with ``best_class`` / ``agnostic_nms``, with ``top_names`` and ``sparse_scores`` (their steps gather the kept rows'
        embeddings like the default one: the two fall out for free) and with per-image banks.  ``prompt_groups=True`` is refused:
        its step is not covered by the tracking tests."""
        from . import track as T
        if self.prompt_groups:
            raise NotImplementedError("track with prompt_groups=True is not implemented; use predict, or a detector without groups")
        n = len(batch_inputs)
        if isinstance(n_seq, bool) or not isinstance(n_seq, int) or n_seq < 1 or n % n_seq:
            raise ValueError(f"n_seq must be a positive int that divides the batch of {n} images, got {n_seq!r}")
        if assignment is not None and assignment not in T.ASSIGNMENTS:
            raise ValueError(f"assignment: one of {T.ASSIGNMENTS} or None is expected, got {assignment!r}")
        if tracker is None:
            if self._tracker is not None and assignment is not None and assignment != self._tracker.assignment:
                raise ValueError(f"assignment {assignment!r} differs from that of the detector's tracker "
                                 f"({self._tracker.assignment!r}): call reset_tracks() first")
            if self._tracker is not None and self._tracker.n_seq != n_seq:
                raise ValueError(f"the detector's tracker holds {self._tracker.n_seq} sequences, this call has {n_seq}: call "
                                 "reset_tracks() first, or pass a tracker")
            if self._tracker is not None and track_params is not None and track_params != self._tracker.params:
                raise ValueError("track_params differ from those of the detector's tracker: call reset_tracks() first")
        elif not isinstance(tracker, T.Tracker) or tracker.n_seq != n_seq or tracker.dim != EMBED_DIM:
            raise ValueError(f"tracker must be a track.Tracker of {n_seq} sequences and dim {EMBED_DIM}")
        elif track_params is not None:
            raise ValueError("track_params belong to the detector's own tracker: a tracker that is passed in carries its own")
        elif assignment is not None:
            raise ValueError("assignment belongs to the detector's own tracker: a tracker that is passed in carries its own")
        res, counts, samples = self._predict_step(batch_inputs, batch_data_samples, rescale, with_embed=True)
        if tracker is None:
            if self._tracker is None:
                self._tracker = T.Tracker(n_seq, dim=EMBED_DIM, params=track_params, device=self._h.device,
                                          assignment=assignment or "greedy")
            tracker = self._tracker
        ids, hits = tracker.update(res, n // n_seq)
        return self._instances(res, counts, samples, (("track_ids", ids), ("track_hits", hits)))

    def reset_tracks(self) -> None:
        """Forget the tracks of ``track``'s own tracker (ids start at 1 again; the next call may use another ``n_seq``)."""
        self._tracker = None

    # -- exemplar prompts --------------------------------------------------------------------
    @torch.no_grad()
    def exemplar_bank(self, batch_inputs, batch_data_samples, exemplars, names=None, *, anchors_per_box: int = 4,
                      min_iou: float = 0.1):
        """Class-bank rows from example boxes instead of text ("find more things like the one in this box").  ``batch_inputs`` /
        ``batch_data_samples`` as in ``predict``; ``exemplars[b]``: the list of ``(box_xyxy_in_original_pixels, class_index)`` of
        image b — the geometry comes from the samples' ``scale_factor`` / ``pad_param`` as in ``predict``.  Every example box takes
        the ``anchors_per_box`` anchors whose decoded boxes overlap it best (IoU > ``min_iou``); a class's row is the IoU-weighted
        mean of their L2-normalised region embeddings, L2-normalised (include/wedetect_hip_exemplar.h).

        Returns ``(bank, info)``: ``bank`` fp32 [C, 768] on the device, unit rows, C = len(names) or the largest class index + 1;
        ``info``: ``names``, ``support`` (anchors pooled per class), ``anchors`` / ``ious`` ([B, max_ex, anchors_per_box] host
        tensors, -1 / 0 in empty slots) and ``examples`` (the (image, example) pairs of every class).

        The rows are used exactly like text rows: ``set_text_embeddings(bank)``, per-image banks, or mixed —
        ``torch.cat([text_bank, exemplar_bank])`` is a valid bank, because text rows are L2-normalised on the device and these
        prototypes are unit rows already.

        ValueError: a box with non-positive width or height, a class index with no example, a class no anchor was assigned to
        (support 0; the message names the class and the best IoU any of its boxes reaches).  The bank is never non-finite: the
        build runs under the range guard of ``predict`` (a trip in fp16x3 repeats it, at last on the fp32 kernels) and a result
        that is non-finite even then raises RuntimeError."""
        plan = plan_exemplars(exemplars, names, anchors_per_box, min_iou)
        dev = self._h.device
        if dev is None:
            raise RuntimeError("model is not on a HIP device: call .cuda()")
        xs = [x for x in batch_inputs]
        samples = list(batch_data_samples) if batch_data_samples is not None else [None] * len(xs)
        if len(samples) != len(xs) or len(exemplars) != len(xs):
            raise ValueError(f"{len(xs)} inputs but {len(samples)} data samples and {len(exemplars)} exemplar lists")
        hh, ww = _batch_hw(xs)
        x = _nhwc_u8(xs, dev)
        tower = self._h.tower(len(xs), hh, ww)
        meta = torch.tensor([letterbox_meta(_meta_of(s), hh, ww, True) for s in samples], dtype=torch.float32, device=dev)
        d = {k: torch.from_numpy(plan[k]).to(dev) for k in ("ex_boxes", "ex_count", "cls_off", "cls_slot")}
        m = plan["m"]
        self._h.calibrate_first(tower, x)
        run = lambda: tower.exemplar_bank(x, meta, d["ex_boxes"], d["ex_count"], d["cls_off"], d["cls_slot"], m, plan["min_iou"])
        res, counts = self._h.checked_run(tower, x, run)
        support = counts[:-1]
        anchors = res["sel_anchors"].view(len(xs), plan["max_ex"], m).cpu()
        ious = res["sel_iou"].view(len(xs), plan["max_ex"], m).cpu()
        for c, n in enumerate(support):
            if n == 0:
                best = self._best_iou(tower, d, meta, plan["cls_examples"][c], plan["max_ex"])
                raise ValueError(f"exemplar class {c} ({plan['names'][c]!r}): no anchor overlaps its example boxes with IoU > "
                                 f"{plan['min_iou']:g} (best IoU {best:.4f}); lower min_iou or check the boxes")
        bank = res["bank"].clone()
        if not bool(torch.isfinite(bank).all()):
            raise RuntimeError("exemplar bank is non-finite after the range guard")
        return bank, dict(names=plan["names"], support=support, anchors=anchors, ious=ious, examples=plan["cls_examples"])

    @staticmethod
    def _best_iou(tower, d: dict, meta: torch.Tensor, examples, max_ex: int) -> float:
        """The largest IoU any anchor reaches with the given (image, example) boxes: the assignment with one anchor and no
        threshold, on the boxes the tower's last head decoded (the error path of ``exemplar_bank`` only)."""
        from . import exemplar as EX
        a = torch.empty(tower.B, max_ex, dtype=torch.int32, device=tower.dev)
        iou, cnt = torch.empty(tower.B, max_ex, dtype=torch.float32, device=tower.dev), torch.empty(tower.B, dtype=torch.int32, device=tower.dev)
        EX.exemplar_assign(tower.boxes, tower.ntot, d["ex_boxes"], d["ex_count"], meta, max_ex, tower.B, 1, 0.0, a, iou, cnt)
        iou = iou.cpu()
        return max(float(iou[b, e]) for b, e in examples)

    def set_exemplar_bank(self, batch_inputs, batch_data_samples, exemplars, names=None, *, anchors_per_box: int = 4,
                          min_iou: float = 0.1):
        """``exemplar_bank(...)`` followed by ``set_text_embeddings(bank, [[n] for n in names])``: the detector then predicts the
        exemplar classes (names default to ``exemplar_<index>``).  Returns ``(bank, info)``."""
        bank, info = self.exemplar_bank(batch_inputs, batch_data_samples, exemplars, names, anchors_per_box=anchors_per_box,
                                        min_iou=min_iou)
        self.set_text_embeddings(bank, [[n] for n in info["names"]])
        return bank, info

    # -- bank tuning --------------------------------------------------------------------
    def tune_bank(self, batch_inputs, batch_data_samples, boxes, names=None, *, init="exemplar", steps: int = 50, lr: float = 1e-2,
                  betas=(0.9, 0.999), eps: float = 1e-8, frozen_rows=None, anchors_per_box: int = 4, min_iou: float = 0.1,
                  fit: bool = True, max_cache_bytes: int = 8 << 30):
        """Learn class-bank rows from labelled boxes with both towers frozen (include/wedetect_hip_tune.h).  ``batch_inputs`` /
        ``batch_data_samples`` as in ``predict``; ``boxes[b]``: the list of ``(box_xyxy_in_original_pixels, class_index)`` of image
        b, the geometry coming from the samples exactly as in ``exemplar_bank``.  The batch's region embeddings and its static
        targets (every box's ``anchors_per_box`` best-overlapping anchors, IoU > ``min_iou``, target = IoU) are cached on the device;
        with ``fit=False`` the call only adds the batch and returns None, so more images than one batch are added by calling it
        repeatedly, and the last call (``fit=True``) runs ``steps`` Adam steps over everything cached and empties the cache.
        ``init`` is used by the fitting call alone (a ``fit=False`` call checks it and computes nothing from it); a call that raises
        leaves the batches added before it in the cache, and ``tune_reset()`` empties the cache.

        ``init``: a [K, 768] bank; ``"text"``, the current text bank; ``"exemplar"``, the pooled prototypes of THE FITTING call's
        boxes (``exemplar_bank``: every class needs a box in that batch, so tuning over several batches wants an explicit bank).
        Class indices are rows of that bank.  ``frozen_rows`` (indices or a bool mask of K) marks rows that serve as negatives only
        — new classes learned beside a text bank: they come back as the normalised start rows, bit for bit (every row of ``init`` is
        L2-normalised once before the first step; normalising a unit row can move an ulp).  ``steps`` and ``lr`` are parameters,
        not tuned values.  A class without a positive anchor is allowed (it learns from negatives only; ``info["no_positive"]``).

        Returns ``(bank, info)``: unit rows fp32 [K, 768], used like any bank (``set_text_embeddings``, per-image banks, every
        detection mode); ``info``: ``names``, ``loss`` (before each step), ``positives`` per class, ``no_positive``, ``plan``,
        ``status``, ``init``.  Detection quality after tuning is unmeasured: no trained weights have been run through this."""
        from . import tune as TN
        if self.prompt_groups:
            raise NotImplementedError("tune_bank with prompt_groups=True is not implemented (it learns one row per class)")
        if isinstance(init, torch.Tensor):
            TN.check_bank(init, "init")
        elif init not in ("text", "exemplar"):
            raise ValueError(f"init: a [K, {EMBED_DIM}] bank, \"text\" or \"exemplar\" is supported, got {init!r}")
        if init == "text":
            if self.text_feats is None:
                raise ValueError("init=\"text\": no text bank is set (reparameterize / set_text_embeddings)")
            TN.check_bank(self.text_feats, "init=\"text\": the current text bank")
        n_rows = None if init == "exemplar" else int((init if isinstance(init, torch.Tensor) else self.text_feats).shape[0])
        if names is not None and n_rows is not None and len(names) != n_rows:
            raise ValueError(f"{len(names)} names for a bank of {n_rows} rows")
        plan = plan_tune_boxes(boxes, n_rows, anchors_per_box, min_iou)
        dev = self._h.device
        if dev is None:
            raise RuntimeError("model is not on a HIP device: call .cuda()")
        xs = [x for x in batch_inputs]
        samples = list(batch_data_samples) if batch_data_samples is not None else [None] * len(xs)
        if len(samples) != len(xs) or len(boxes) != len(xs):
            raise ValueError(f"{len(xs)} inputs but {len(samples)} data samples and {len(boxes)} box lists")
        bank0 = None
        if not fit:
            pass                                             # only the fitting call's init is used: nothing to compute here
        elif init == "exemplar":
            bank0, _ = self.exemplar_bank(batch_inputs, batch_data_samples, boxes, names, anchors_per_box=anchors_per_box, min_iou=min_iou)
        elif init == "text":
            bank0 = self.text_feats
        else:
            bank0 = init.to(dev)
        hh, ww = _batch_hw(xs)
        x = _nhwc_u8(xs, dev)
        tower = self._h.tower(len(xs), hh, ww)
        meta = torch.tensor([letterbox_meta(_meta_of(s), hh, ww, True) for s in samples], dtype=torch.float32, device=dev)
        d = {k: torch.from_numpy(plan[k]).to(dev) for k in ("ex_boxes", "ex_count", "gt_cls")}
        tuner = self._tuner
        if tuner is None:
            tuner = self._tuner = TN.BankTuner(tower, max_cache_bytes)
        tuner.max_cache_bytes = int(max_cache_bytes)
        self._h.calibrate_first(tower, x)
        first = len(tuner.chunks)

        def run():
            tuner.truncate(first)                            # a repeat under the range guard replaces the chunk
            c = tuner.add_batch(x, meta, d["ex_boxes"], d["ex_count"], d["gt_cls"], plan["m"], plan["min_iou"], tower=tower)
            bad = ~torch.isfinite(c["E"]).all()
            return dict(count=torch.cat([c["sel_count"], -bad.to(torch.int32).view(1)]))
        try:
            with torch.no_grad():
                self._h.checked_run(tower, x, run)
        except BaseException:
            tuner.truncate(first)                            # the cache holds whole batches only
            raise
        if not fit:
            return None
        K = int(bank0.shape[0])
        trainable = torch.ones(K, dtype=torch.bool)
        if frozen_rows is not None:
            fr = torch.as_tensor(frozen_rows)
            if fr.dtype == torch.bool:
                if tuple(fr.shape) != (K,):
                    raise ValueError(f"frozen_rows: a bool mask of {K} rows is supported, got {tuple(fr.shape)}")
                trainable = ~fr.cpu()
            else:
                if fr.numel() and (int(fr.min()) < 0 or int(fr.max()) >= K):
                    raise ValueError(f"frozen_rows: indices in 0 .. {K - 1} are supported")
                trainable[fr.to(torch.int64).cpu()] = False
        try:
            with torch.no_grad():
                bank, info = tuner.fit(bank0, steps, lr=lr, betas=betas, eps=eps, trainable=trainable)
        finally:
            self._tuner = None                               # the cache is spent either way
        if not bool(torch.isfinite(bank).all()):
            raise RuntimeError("tuned bank is non-finite")
        info["names"] = [str(n) for n in names] if names is not None else [f"{'exemplar' if init == 'exemplar' else 'class'}_{c}" for c in range(K)]
        for k in ("w", "m", "v"):
            info.pop(k)
        info["init"] = bank0.detach().clone()                # the rows the steps started from, before normalisation
        return bank, info

    def tune_reset(self) -> None:
        """Drop the batches ``tune_bank(..., fit=False)`` has cached."""
        self._tuner = None

    def set_tuned_bank(self, batch_inputs, batch_data_samples, boxes, names=None, **kw):
        """``tune_bank(...)`` followed by ``set_text_embeddings(bank, [[n] for n in names])``.  Returns ``(bank, info)``."""
        if kw.get("fit", True) is False:
            raise ValueError("set_tuned_bank fits: add earlier batches with tune_bank(..., fit=False)")
        bank, info = self.tune_bank(batch_inputs, batch_data_samples, boxes, names, **kw)
        self.set_text_embeddings(bank, [[n] for n in info["names"]])
        return bank, info

    def predict_stream(self, data_infos: Sequence[dict], batch_size: int, pipeline_cfg, *, rescale: bool = True,
                       decode_workers: Optional[int] = None, stats: Optional[dict] = None):
        """``predict`` over a whole list of data infos (``dataset.get_data_info(i)``: ``img_path``, ``img_id``, optionally
        ``texts``) as a stream of batches (wedetect_amd/stream.py).  ``pipeline_cfg``: the test pipeline (the config's list
        of dicts or a ``Compose``) — it must have the shipped shape (LoadImageFromFile, WeDetectKeepRatioResize,
        WeDetectLetterResize, LoadAnnotations, LoadText, PackDetInputs); its geometry code runs as it is, its pixel work is
        replaced by ONE batched launch sequence per batch.  Yields one ``DetDataSample`` per image, in input order, each
        exactly once; ``pred_instances`` holds what ``predict`` fills, as HOST tensors.  ``stats``: a dict that receives
        the stream's counters when it ends."""
        self._refuse_top_names("predict_stream")
        self._refuse_sparse("predict_stream")
        self._refuse_groups("predict_stream")
        from .stream import MmdetBackend, predict_stream
        return predict_stream(MmdetBackend(self, pipeline_cfg, rescale), data_infos, batch_size, decode_workers, stats)

    # -- tiled inference --------------------------------------------------------------------
    def _best_kw(self) -> dict:
        """The single-label keywords of a tower step; empty for the multi-label default (graph keys stay as they were)."""
        return dict(best_class=True, agnostic_nms=self.agnostic_nms) if self.best_class else {}

    def _refuse_top_names(self, what: str) -> None:
        if self.top_names:
            raise NotImplementedError(f"{what} with top_names={self.top_names} is not implemented (its packed result blobs do not "
                                      "carry the name lists; use predict)")

    def _refuse_groups(self, what: str) -> None:
        if self.prompt_groups:
            raise NotImplementedError(f"{what} with prompt_groups=True is not implemented (its steps score one row per class; use "
                                      "predict)")

    def _refuse_best(self, what: str) -> None:
        self._refuse_top_names(what)
        self._refuse_groups(what)
        if self.best_class:
            raise NotImplementedError(f"{what} with best_class=True is not implemented (the merges rank (anchor, class) candidates)")
        self._refuse_sparse(what)

    def _sparse_kw(self) -> dict:
        """The sparse-score keywords of a tower step; empty for the default (graph keys stay as they were)."""
        return dict(sparse_scores=True, sparse_cap=self.sparse_cap) if self.sparse_scores else {}

    def _refuse_sparse(self, what: str) -> None:
        if self.sparse_scores:
            raise NotImplementedError(f"{what} with sparse_scores=True is not implemented (its packed result blobs do not carry "
                                      "the sparse status; use predict)")

    def _step_kw(self, modes: bool = False) -> dict:
        """The keywords of this detector's tower steps (mmdet ``_bbox_post_process`` -> ``mmcv.ops.batched_nms(bboxes, scores,
        labels, cfg.nms)``).  ``modes``: with the keywords of the modes that are ON (``predict``; the plan of prompt groups
        belongs to a bank and is added there) — a mode that is off adds nothing, so graph keys stay as they were."""
        cfg = self.test_cfg
        kw = dict(normalize_text=True, score_thr=cfg["score_thr"], iou_thr=cfg["nms"]["iou_threshold"], with_embed=False,
                  nms="mmcv", nms_param=int(cfg["nms"].get("split_thr", 10000)))
        if modes:
            kw.update(self._best_kw(), **self._sparse_kw(), **(dict(top_names=self.top_names) if self.top_names else {}))
        return kw

    @torch.no_grad()
    def predict_tiled(self, image, texts=None, *, tile=None, overlap: float = 0.2, overview: bool = True, tile_batch: int = 32,
                      edge_margin: float = 2.0, merge_iou: Optional[float] = None, max_per_img: Optional[int] = None,
                      channel_order: str = "rgb", stats: Optional[dict] = None) -> "DetDataSample":
        """One LARGE image at the network's own resolution: cut into overlapping ``tile``-sized crops (+ one overview of the
        whole image through the test pipeline's geometry), detected as batches of ``tile_batch`` tiles, merged on the device
        (wedetect_amd/tiling.py, include/wedetect_hip_tile.h):

            upload (image, plan + metadata) -> ONE cut launch (+ the overview's resize) -> pipelined tower steps
            (``detect(overlap_post=True)``; each step's rows are copied into stacked buffers on the post stream) -> ONE merge
            (border drop, translate, sort, mmcv-form NMS over all tiles) -> ONE download (rows, count, range flags)

        ``image``: HWC uint8 (ndarray / tensor, host or device) or a PIL image, channels in ``channel_order`` ("rgb" / "bgr").
        ``texts``: a class list ``[[a], [b], ...]`` (None: the bank of ``reparameterize`` / ``set_text_embeddings``).
        ``tile`` (h, w), None = ``img_scale``; ``merge_iou`` None = ``test_cfg.nms.iou_threshold``; ``max_per_img`` None =
        ``test_cfg.max_per_img``; ``edge_margin``: rows closer than this to an INTERIOR side of their crop are dropped (the
        object is cut there and lies whole in a neighbouring crop or in the overview).  A remainder of r tiles runs on the
        tower of the next power of two >= r, padded with blank tiles.  An image that fits one tile goes through ``predict``.

        The pipelined steps only DETECT a trip of the fp16x3 range guard (a flag, or a count of -1, arrives with the
        download); the image is then run again step by step in line through ``checked_counts``, which owns the guard's logic,
        the protocol of wedetect_amd/guarded.py.  Returns a ``DetDataSample`` whose ``pred_instances`` holds HOST tensors: ``bboxes``
        (image pixels), ``scores``, ``labels`` and ``tiles`` (the plan index of the tile each row came from)."""
        self._refuse_best("predict_tiled")
        from . import tile as T
        from . import tiling as G
        from .pipeline import cv_resize_pad
        dev = self._h.device
        if dev is None:
            raise RuntimeError("model is not on a HIP device: call .cuda()")
        if channel_order not in ("rgb", "bgr"):
            raise ValueError("channel_order must be 'rgb' or 'bgr'")
        swap = channel_order == "bgr"                        # the tower reads RGB
        if hasattr(image, "convert") and not isinstance(image, (np.ndarray, torch.Tensor)):
            image = np.asarray(image.convert("RGB"))
        img = torch.from_numpy(np.ascontiguousarray(image)) if isinstance(image, np.ndarray) else image
        if not isinstance(img, torch.Tensor) or img.dtype != torch.uint8 or img.dim() != 3 or img.shape[2] != 3:
            raise TypeError("image must be uint8 HxWx3")
        H, W = int(img.shape[0]), int(img.shape[1])
        th, tw = (int(v) for v in (tile if tile is not None else self.img_scale))
        max_out = int(max_per_img if max_per_img is not None else self.test_cfg["max_per_img"])
        if not 1 <= max_out <= T.MERGE_MAX_OUT:
            raise NotImplementedError(f"max_per_img {max_out} outside 1 .. {T.MERGE_MAX_OUT} (the NMS kernel's kept-list capacity)")
        iou = float(merge_iou if merge_iou is not None else self.test_cfg["nms"]["iou_threshold"])
        if not float(edge_margin) >= 0.0:
            raise ValueError("edge_margin must be >= 0")
        plan = G.plan_tiles(H, W, (th, tw), overlap, overview)
        sample = DetDataSample(metainfo=dict(ori_shape=(H, W), img_shape=(H, W)))
        if texts is not None:
            sample.set_metainfo(dict(texts=texts))
        bank = self._bank_for(sample).to(dev)
        if stats is not None:
            stats.update(tiles=len(plan), crops=G.n_crops(plan), steps=0, trips=0, inline=False, d2h_copies=0)
        img_dev = img.to(dev, non_blocking=True).contiguous()
        if G.fits_one_tile(plan):
            # the plain step: the image through the test pipeline's geometry, then ``predict``
            g = G.overview_geometry(H, W, (th, tw))
            canvas = cv_resize_pad(img_dev, g["dh"], g["dw"], g["interp"], (th, tw), g["top"], g["left"], g["pad_val"], swap_rb=not swap)
            sample.set_metainfo(dict(scale_factor=g["scale_factor"], pad_param=g["pad_param"], img_shape=(th, tw, 3)))
            return self.predict([canvas.permute(2, 0, 1).contiguous()], [sample])[0]          # predict takes CHW BGR
        h = self._h
        sizes = G.step_sizes(len(plan), tile_batch)
        total = sum(b for _, b in sizes)
        max_in = h.max_out
        if total * max_in > T.MERGE_MAX_ROWS:
            raise NotImplementedError(f"{total} tiles x {max_in} rows per tile exceed the merge's {T.MERGE_MAX_ROWS} rows: use larger "
                                      "tiles, less overlap or a smaller test_cfg.max_per_img")
        plan_p = G.pad_plan(plan, total)
        og = G.overview_geometry(H, W, (th, tw)) if bool((plan["kind"] == G.OVERVIEW).any()) else None
        B = self._tiled_buffers(total, max_in, th, tw, max_out, len(sizes), dev)
        # ONE control block: descriptors, then the per-tile metadata at a 256-byte boundary
        ctl_host = B["ctl_io"].host                          # the previous call ended with a synchronisation: free to rewrite
        ctl_host["plan"].numpy()[:] = plan_p.view(np.uint8)
        ctl_host["meta"].numpy()[:] = G.tile_meta(plan_p, (th, tw), None if og is None else og["meta"])
        B["ctl_io"].upload()
        ctl, meta, tiles = B["ctl"], B["ctl_io"].views["meta"], B["tiles"]
        T.tile_cut_u8(img_dev, ctl.data_ptr(), plan_p, tiles, fill=114, swap_rb=swap)
        if og is not None:
            k = int(np.nonzero(plan_p["kind"] == G.OVERVIEW)[0][0])
            cv_resize_pad(img_dev, og["dh"], og["dw"], og["interp"], (th, tw), og["top"], og["left"], og["pad_val"], swap_rb=swap,
                          out=tiles[k])
        n_cls = int(bank.shape[0])
        split_thr = int(self.test_cfg["nms"].get("split_thr", 10000))
        steps, lo = [], 0
        for i, (_, b) in enumerate(sizes):                   # destination: the step's flag row and its rows of the stacked buffers
            steps.append((h.tower(b, th, tw), tiles[lo:lo + b], bank, None, meta[lo:lo + b], i, slice(lo, lo + b)))
            lo += b

        def merge_and_download():
            T.tile_merge(B["boxes"], B["scores"], B["labels"], B["counts"], ctl.data_ptr(), total, max_in, n_cls, float(edge_margin),
                         iou, split_thr, max_out, B["out_boxes"], B["out_scores"], B["out_labels"], B["out_src"], B["out_count"], B["ws"])
            if stats is not None:
                stats["d2h_copies"] += 1
            return B["out_io"].fetch()                       # ONE packed D2H: rows, count, range flags

        host = run_steps(h, steps, self._step_kw(), B, merge_and_download, stats)
        n = int(host["out_count"])
        sample.pred_instances = InstanceData(bboxes=host["out_boxes"][:n], scores=host["out_scores"][:n],
                                             labels=host["out_labels"][:n].to(torch.int64),
                                             tiles=(host["out_src"][:n] // max_in).to(torch.int64))
        return sample

    def _tiled_buffers(self, total: int, max_in: int, th: int, tw: int, max_out: int, n_steps: int, dev) -> dict:
        """Device buffers of ``predict_tiled`` for one geometry, kept between calls: the tiles, the stacked per-tile rows, the
        merge's workspace, ONE control block (``ctl_io``: descriptors, per-tile metadata) and ONE staging blob (``out_io``:
        merged rows, count, range flags per step), each a ``guarded.Blob`` whose device parts are entries of their own."""
        from . import tile as T
        key = (total, max_in, th, tw, max_out, n_steps, str(dev))
        B = getattr(self, "_tiled", None)
        if B is not None and B["key"] == key:
            return B
        f32, i32, u8 = torch.float32, torch.int32, torch.uint8
        e = lambda *s, dt=f32: torch.empty(*s, dtype=dt, device=dev)
        B = dict(key=key, tiles=e(total, th, tw, 3, dt=u8), boxes=e(total, max_in, 4), scores=e(total, max_in),
                 labels=e(total, max_in, dt=i32), counts=e(total, dt=i32),
                 ws=e(T.merge_workspace_bytes(total, max_in), dt=u8), events=[torch.cuda.Event() for _ in range(n_steps)])
        B["ctl_io"], B["out_io"] = Blob(_tiled_ctl_parts(total), dev), Blob(merged_parts(max_out, n_steps), dev)
        B.update(B["out_io"].views, ctl=B["ctl_io"].dev, stage=B["out_io"].dev)
        self._tiled = B
        return B

    # -- test-time augmentation -------------------------------------------------------------
    @torch.no_grad()
    def predict_views(self, views, tta_cfg: dict, rescale: bool = True, stats: Optional[dict] = None) -> List["DetDataSample"]:
        """Test-time augmentation of one batch (mmdet ``DetTTAModel``; wedetect_amd/tta.py, include/wedetect_hip_views.h).
        ``views``: a list of ``(batch_inputs, batch_data_samples)`` as ``predict`` takes them, one per view, all of the same B
        images in the same order; a view's samples say how it was flipped (``flip`` / ``flip_direction``).  Every view has one
        input shape; at most 4 distinct shapes (the towers kept per shape).  ``tta_cfg``:
        ``dict(nms=dict(type='nms', iou_threshold=...[, split_thr]), max_per_img=...)``.

            one pipelined tower step per view (``detect(overlap_post=True)`` with ``predict``'s keywords, per-image banks
            included; each step's rows are copied into stacked [V, B, max_in] buffers on the post stream) -> ONE merge
            (``wd_views_merge``: un-flip, sort, mmcv-form NMS per image over all views) -> ONE download (rows, counts, flags)

        The pipelined steps only DETECT a trip of the fp16x3 range guard (wedetect_amd/guarded.py): the views are then run again
        in line through ``checked_counts`` and merged again.  Returns the FIRST view's sample of every image (mmdet
        ``_merge_single_sample``); ``pred_instances`` holds HOST tensors: ``bboxes`` (original-image pixels), ``scores``,
        ``labels`` and ``views`` (the view each row came from)."""
        self._refuse_best("predict_views")
        from . import views as VW
        from .tta import check_tta_cfg
        h = self._h
        dev = h.device
        if dev is None:
            raise RuntimeError("model is not on a HIP device: call .cuda()")
        cfg = check_tta_cfg(tta_cfg)
        views = [(list(x for x in inp), list(smp) if smp is not None else [None] * len(inp)) for inp, smp in views]
        V = len(views)
        if not 1 <= V <= VW.MERGE_MAX_VIEWS:
            raise NotImplementedError(f"{V} views: 1 .. {VW.MERGE_MAX_VIEWS} are supported")
        B = len(views[0][0])
        max_in, max_out = h.max_out, cfg["max_per_img"]
        if V * max_in > VW.MERGE_MAX_ROWS:
            raise NotImplementedError(f"{V} views x {max_in} rows per view exceed the merge's {VW.MERGE_MAX_ROWS} rows per image: use "
                                      "fewer views or a smaller test_cfg.max_per_img")
        shapes, flips, banks_v = [], [], []
        for v, (xs, samples) in enumerate(views):
            if len(xs) != B or len(samples) != B or B < 1:
                raise ValueError(f"view {v}: {len(xs)} inputs and {len(samples)} data samples, but view 0 has {B} images")
            shapes.append(_batch_hw(xs, f"view {v}: "))
            codes = set()
            for s in samples:
                m = _meta_of(s)
                d = m.get("flip_direction") if m.get("flip") else None
                if d not in VW.FLIP_CODES:
                    raise ValueError(f"view {v}: flip_direction {d!r}")
                codes.add(VW.FLIP_CODES[d])
            if len(codes) != 1:
                raise ValueError(f"view {v}: its samples disagree about the flip ({sorted(codes)}); a view is one augmentation of the batch")
            flips.append(codes.pop())
            banks_v.append([self._bank_for(s) for s in samples])
        if len(set(shapes)) > 4:
            raise NotImplementedError(f"{len(set(shapes))} distinct input shapes: at most 4 (one tower is kept per shape)")
        n_cls = max(int(b.shape[0]) for banks in banks_v for b in banks)
        iou, split_thr = cfg["nms"]["iou_threshold"], int(cfg["nms"].get("split_thr", 10000))
        Bf = self._views_buffers(V, B, max_in, max_out, tuple(shapes), dev)
        ctl = Bf["ctl_io"].host                              # the previous call ended with a synchronisation: free to rewrite
        ctl["flip"][:] = torch.tensor(flips, dtype=torch.int32)
        for b, s in enumerate(views[0][1]):
            ori = _meta_of(s).get("ori_shape", shapes[0])
            ctl["wh"][b, 0], ctl["wh"][b, 1] = float(ori[1]), float(ori[0])
        for v, (_, samples) in enumerate(views):
            ctl["meta"][v] = torch.tensor([letterbox_meta(_meta_of(s), shapes[v][0], shapes[v][1], rescale) for s in samples],
                                          dtype=torch.float32)
        Bf["ctl_io"].upload()
        towers = [h.tower(B, hh, ww) for hh, ww in shapes]
        packed = [self._packed_for(banks, dev) for banks in banks_v]
        text = [(banks[0].to(dev), None) if p is None else p for banks, p in zip(banks_v, packed)]
        for v, (xs, _) in enumerate(views):
            _nhwc_u8(xs, dev, out=Bf["x"][v])                # as predict
        if stats is not None:
            stats.update(views=V, steps=0, trips=0, inline=False, d2h_copies=0)
        steps = [(towers[v], Bf["x"][v], text[v][0], text[v][1], Bf["meta"][v], v, v) for v in range(V)]

        def merge_and_download():
            VW.views_merge(Bf["boxes"], Bf["scores"], Bf["labels"], Bf["counts"], Bf["flip"], Bf["wh"], V, B, max_in, n_cls, iou, split_thr,
                           max_out, Bf["out_boxes"], Bf["out_scores"], Bf["out_labels"], Bf["out_src"], Bf["out_count"], Bf["ws"])
            if stats is not None:
                stats["d2h_copies"] += 1
            return Bf["out_io"].fetch()                      # ONE packed D2H: rows, counts, range flags

        host = run_steps(h, steps, self._step_kw(), Bf, merge_and_download, stats)
        out = []
        for b, s in enumerate(views[0][1]):
            n = int(host["out_count"][b])
            s = _as_sample(s)
            s.pred_instances = InstanceData(bboxes=host["out_boxes"][b, :n], scores=host["out_scores"][b, :n],
                                            labels=host["out_labels"][b, :n].to(torch.int64),
                                            views=(host["out_src"][b, :n] // max_in).to(torch.int64))
            out.append(s)
        return out

    def _views_buffers(self, V: int, B: int, max_in: int, max_out: int, shapes: tuple, dev) -> dict:
        """Device buffers of ``predict_views`` for one geometry, kept between calls: the NHWC input of every view, the stacked
        per-view rows, the merge's workspace, ONE control block (``ctl_io``: flip codes, image sizes, per-view metadata) and ONE
        staging blob (``out_io``: merged rows, counts, range flags per view), each a ``guarded.Blob`` whose device parts are
        entries of their own."""
        from . import views as VW
        key = (V, B, max_in, max_out, shapes, str(dev))
        Bf = getattr(self, "_views", None)
        if Bf is not None and Bf["key"] == key:
            return Bf
        f32, i32, u8 = torch.float32, torch.int32, torch.uint8
        e = lambda *s, dt=f32: torch.empty(*s, dtype=dt, device=dev)
        Bf = dict(key=key, x=[e(B, hh, ww, 3, dt=u8) for hh, ww in shapes], boxes=e(V, B, max_in, 4), scores=e(V, B, max_in),
                  labels=e(V, B, max_in, dt=i32), counts=e(V, B, dt=i32), ws=e(VW.merge_workspace_bytes(V, B, max_in), dt=u8),
                  events=[torch.cuda.Event() for _ in range(V)])
        Bf["ctl_io"], Bf["out_io"] = Blob(_views_ctl_parts(V, B), dev), Blob(merged_parts(max_out, V, (B,)), dev)
        Bf.update(Bf["ctl_io"].views, **Bf["out_io"].views, ctl=Bf["ctl_io"].dev, stage=Bf["out_io"].dev)
        self._views = Bf
        return Bf


MODELS.register_module(module=YOLOWorldDetector)
MODELS.register_module(module=MultiModalYOLOBackbone)
