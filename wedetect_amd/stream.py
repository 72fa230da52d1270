"""Streamed dataset inference: decode threads -> pinned arenas -> one batched feed launch sequence -> pipelined tower
steps -> one packed result copy per batch.

    decode threads :  decode batch i+2 into the pinned arena slot
    upload stream  :  H2D pixels i+1, H2D control block i+1
    download stream:  D2H results i-1 (one packed copy)
    tower          :  feed kernels i -> detect(overlap_post=True) i   (backbone | neck + head | post on their streams)

Uploads and downloads have a stream each: the download of step i waits for that step's post-process, and an upload queued
behind it on the same in-order stream would hold the feed and the backbone of step i+1 back until step i had finished.  On
its own stream the upload of batch i+1 waits only for the feed kernels of batch i-1 (the last readers of its device arenas),
so it — and the backbone of step i+1 behind it — runs beside the neck, head and post-process of step i.  The issuing thread
never waits for an upload either: a pinned slot is handed to the decode threads at once, and each of them waits for the
slot's last upload itself, after it has decoded its image and before it writes the pixels into the slot.

Two layers:

``StreamScheduler``   the ordering alone — which batch is decoded, uploaded, issued and read when; bounded depth (at most two
                      batches issued and unread), drain at a batch of another size, decode errors raised in the consumer
                      with the path, the range-guard detour (discard what is in flight, run the batch in line, re-issue).
                      It talks to a backend through seven methods and never touches a device: tests/test_cpu_feed.py drives it
                      with a stub.
``TowerBackend``      the device side for the two detectors (``MmdetBackend`` for ``YOLOWorldDetector.predict_stream``,
                      ``UniBackend`` for ``SimpleYOLOWorldDetector.predict_stream``): two pinned and two device arenas
                      (pixels + control block = descriptors, tables, letterbox metadata), one tmp arena, two result staging
                      sets, all grown geometrically to the largest batch seen and otherwise never allocated per step.

The range guard follows the guarded-step protocol of wedetect_amd/guarded.py, with the scheduler in the place of its driver: a
streamed step only DETECTS a trip (flags and -1 counts arrive with its results); the batch is then run again in line, from the
canvas the feed already wrote, and while a tower is in its fp32 fallback every batch goes in line, so that the counters and the
tower state follow exactly the sequence the serial loop produces.
"""
from __future__ import annotations

import functools
import os
import threading
from collections import deque
from concurrent.futures import ThreadPoolExecutor
from typing import Dict, Iterator, List, Optional, Sequence

import numpy as np

MAX_DECODE_WORKERS = 12
DEPTH = 2                        # batches issued and not yet read


def decode_pool_size(decode_workers: Optional[int] = None) -> int:
    """``min(12, $OMP_NUM_THREADS or 8)`` unless the caller says otherwise; never derived from the machine's CPU count (a
    shared host shows many times the CPUs a job may use)."""
    if decode_workers is not None:
        n = int(decode_workers)
        if n < 1:
            raise ValueError("decode_workers must be positive")
        return min(n, MAX_DECODE_WORKERS)
    try:
        n = int(os.environ.get("OMP_NUM_THREADS", "") or 8)
    except ValueError:
        n = 8
    return max(1, min(MAX_DECODE_WORKERS, n))


class DecodeError(RuntimeError):
    pass


def _name_of(item) -> str:
    if isinstance(item, dict):
        return str(item.get("img_path", item.get("img_id", "<image>")))
    return item if isinstance(item, str) else f"<{type(item).__name__}>"


class StreamScheduler:
    """``for result in StreamScheduler(backend, batch_size).run(items)``: one result per item, in input order, each once.

    Backend protocol (``slot`` is 0 or 1 = batch index & 1):
      ``decode(item, slot)``            worker thread: decode one item into the slot's input arena, return its geometry
      ``input_free(slot)``              main thread: the slot's input arena is about to take another batch; reset it (a backend
                                        whose previous upload may still be reading it makes ``decode`` wait, not this call)
      ``upload(slot, items, geoms)``    stage the batch's device inputs (asynchronous)
      ``issue(slot)``                   issue the step of the uploaded batch (asynchronous)
      ``collect(slot)``                 block for the issued step's results -> (tripped, [result per item])
      ``inline(slot)``                  run the uploaded batch through the in-line path -> [result per item]
      ``inline_only()``                 True while every batch must go in line (a tower in its fp32 fallback)
      ``drain()``                       block until nothing is in flight; what was issued and not collected is discarded
    """

    def __init__(self, backend, batch_size: int, decode_workers: Optional[int] = None):
        if batch_size < 1:
            raise ValueError("batch_size must be positive")
        self.backend, self.batch_size = backend, int(batch_size)
        self.workers = decode_pool_size(decode_workers)
        self.stats: Dict[str, int] = dict(batches=0, max_in_flight=0, trips=0, inline_batches=0, reissued=0)

    def run(self, items: Sequence) -> Iterator:
        items = list(items)
        bs, be = self.batch_size, self.backend
        batches = [items[k:k + bs] for k in range(0, len(items), bs)]
        n = len(batches)
        if n == 0:
            return
        pool = ThreadPoolExecutor(max_workers=self.workers, thread_name_prefix="wd-decode")
        futures: Dict[int, list] = {}
        uploaded = set()

        def submit(k):                                   # decode batch k into slot k & 1
            if k < n and k not in futures:
                be.input_free(k & 1)
                futures[k] = [pool.submit(be.decode, it, k & 1) for it in batches[k]]

        def upload(k):
            if k < n and k not in uploaded:
                geoms = []
                for it, f in zip(batches[k], futures[k]):
                    try:
                        geoms.append(f.result())
                    except Exception as e:               # raised here, in the consumer, with the path
                        raise DecodeError(f"decoding {_name_of(it)} failed: {type(e).__name__}: {e}") from e
                be.upload(k & 1, batches[k], geoms)
                uploaded.add(k)
                futures[k] = []
                submit(k + 2)                            # the pinned slot is free once this upload has been read

        pending: deque = deque()                         # issued, not collected (oldest first)

        def done(j):
            """Batch j has its results: its slot's device arenas may take batch j + 2."""
            self.stats["batches"] += 1
            upload(j + 2)

        try:
            submit(0)
            submit(1)
            i = 0                                        # next batch to issue
            while i < n or pending:
                # read the oldest issued step when nothing more may be issued: the depth is reached (step i - 1 is read only
                # after step i has been issued), the input is exhausted, the next batch has another size (the tail switches
                # tower) or must go in line
                if pending and (i >= n or len(pending) >= DEPTH or be.inline_only() or len(batches[i]) != len(batches[pending[-1]])):
                    j = pending.popleft()
                    tripped, res = be.collect(j & 1)
                    if tripped:                          # discard what was issued after it, run j in line, issue the rest again
                        self.stats["trips"] += 1
                        be.drain()
                        if pending:
                            i = pending[0]
                            self.stats["reissued"] += len(pending)
                            pending.clear()
                        res = be.inline(j & 1)
                        self.stats["inline_batches"] += 1
                    if len(res) != len(batches[j]):
                        raise RuntimeError(f"backend returned {len(res)} results for a batch of {len(batches[j])}")
                    yield from res
                    done(j)
                    continue
                upload(i)                                # already done at done(i - 2) except for the first two batches
                if be.inline_only():
                    res = be.inline(i & 1)
                    self.stats["inline_batches"] += 1
                    if len(res) != len(batches[i]):
                        raise RuntimeError(f"backend returned {len(res)} results for a batch of {len(batches[i])}")
                    yield from res
                    i += 1
                    done(i - 1)
                    continue
                be.issue(i & 1)
                pending.append(i)
                self.stats["max_in_flight"] = max(self.stats["max_in_flight"], len(pending))
                i += 1
        finally:
            for fs in futures.values():
                for f in fs:
                    f.cancel()
            pool.shutdown(wait=True)
            be.drain()


# ==================================================================================================
# device backend
# ==================================================================================================
class _Slot:
    def __init__(self):
        self.pin_px = self.pin_px_np = self.pin_ctl = self.pin_ctl_np = None
        self.dev_px = self.dev_ctl = self.canvas = None
        self.stage = self.pin_out = None
        self.lock = threading.Lock()
        self.top = 0
        self.ev_up = self.ev_free = self.ev_staged = self.ev_d2h = None
        self.ctx: Optional[dict] = None


def _no_grad(fn):
    """``torch.no_grad()`` around one backend call (a ``with`` inside the generator would leak into the consumer between
    yields)."""
    @functools.wraps(fn)
    def wrapped(*a, **kw):
        import torch
        with torch.no_grad():
            return fn(*a, **kw)
    return wrapped


def _grow(need: int, have: int) -> int:
    return max(int(need), 2 * int(have), 1 << 20)


class TowerBackend:
    """Device side of the streamed loader for a detector with a ``_TowerHolder`` (``det._h``).  Subclasses give the geometry
    of an image (``plan``), the step's keywords (``step_kw``), its text operands (``texts``) and the per-image result
    (``result``)."""

    RESULT_KEYS = ("bboxes", "scores", "labels", "count")

    def __init__(self, det):
        import torch
        self.det, self.h = det, det._h
        if self.h.device is None:
            raise RuntimeError("model is not on a HIP device: call .cuda()")
        self.dev = self.h.device
        self.slots = [_Slot(), _Slot()]
        self.tmp = None
        self.up_stream = torch.cuda.Stream(device=self.dev)       # H2D of batch i + 1: waits for the feed of batch i - 1 only
        self.down_stream = torch.cuda.Stream(device=self.dev)     # D2H of step i: waits for that step's post-process
        for s in self.slots:
            s.ev_up, s.ev_free, s.ev_staged, s.ev_d2h = (torch.cuda.Event() for _ in range(4))
        # every counter is incremented where this module issues the copy or the launch (``_tally``), per batch; a step that is
        # issued again after a trip counts what it really issues again (the feed, the download), not the upload
        self.stats: Dict[str, int] = dict(steps=0, feed_launches=0, h2d_copies=0, d2h_copies=0, feed_launches_max=0,
                                          h2d_copies_max=0, d2h_copies_max=0, tables_packed=0, arena_grows=0)

    # ------------------------------------------------------------------ hooks
    def load(self, item):
        """Worker thread: -> uint8 HWC RGB ndarray of the item."""
        raise NotImplementedError

    def plan(self, item, h: int, w: int) -> dict:
        """-> dict(plan=feed plan, canvas=(H, W), meta=[8 floats], ...whatever ``result`` needs)."""
        raise NotImplementedError

    def texts(self, ctx):
        """-> (text tensor, device counts or None) of the batch."""
        raise NotImplementedError

    def step_kw(self) -> dict:
        raise NotImplementedError

    def result(self, ctx, j: int, host: Dict[str, "object"], n: int, tower):
        raise NotImplementedError

    # ------------------------------------------------------------------ decode (worker threads)
    def decode(self, item, slot: int):
        s = self.slots[slot]
        a = self.load(item)
        if a.dtype != np.uint8 or a.ndim != 3 or a.shape[2] != 3:
            raise TypeError("images must be uint8 HxWx3")
        h, w = int(a.shape[0]), int(a.shape[1])
        if h < 1 or w < 1:
            raise ValueError("empty image")
        nbytes = h * w * 3
        with s.lock:                                     # reserve a 256-byte aligned range of the pinned arena
            off = s.top
            fits = s.pin_px_np is not None and off + nbytes <= s.pin_px_np.size
            if fits:
                s.top = (off + nbytes + 255) // 256 * 256
        if not fits:
            return dict(h=h, w=w, off=None, spill=np.ascontiguousarray(a))     # the main thread grows the arena and places it
        s.ev_up.synchronize()                            # the slot's previous upload has read the pinned arena (no-op before the first)
        np.copyto(s.pin_px_np[off:off + nbytes].reshape(h, w, 3), a)
        return dict(h=h, w=w, off=off, spill=None)

    def input_free(self, slot: int) -> None:
        self.slots[slot].top = 0                         # ``decode`` waits for the slot's last upload before it writes

    # ------------------------------------------------------------------ arenas
    def _pinned(self, nbytes: int):
        import torch
        t = torch.empty(int(nbytes), dtype=torch.uint8).pin_memory()
        return t, t.numpy()

    def _ensure(self, s: _Slot, px_bytes: int, ctl_bytes: int, tmp_bytes: int) -> None:
        import torch
        grew = False
        if s.pin_px is None or s.pin_px.numel() < px_bytes:
            old, used = s.pin_px_np, s.top
            s.pin_px, s.pin_px_np = self._pinned(_grow(px_bytes, 0 if s.pin_px is None else s.pin_px.numel()))
            if old is not None and used:
                s.pin_px_np[:used] = old[:used]
            grew = True
        if s.pin_ctl is None or s.pin_ctl.numel() < ctl_bytes:
            s.pin_ctl, s.pin_ctl_np = self._pinned(_grow(ctl_bytes, 0 if s.pin_ctl is None else s.pin_ctl.numel()))
            grew = True
        if s.dev_px is None or s.dev_px.numel() < s.pin_px.numel() or s.dev_ctl.numel() < s.pin_ctl.numel() or \
                self.tmp is None or self.tmp.numel() < tmp_bytes:
            torch.cuda.synchronize(self.dev)             # rare (geometric growth): nothing in flight may still use the old ones
            if s.dev_px is None or s.dev_px.numel() < s.pin_px.numel():
                s.dev_px = torch.empty(s.pin_px.numel(), dtype=torch.uint8, device=self.dev)
            if s.dev_ctl is None or s.dev_ctl.numel() < s.pin_ctl.numel():
                s.dev_ctl = torch.empty(s.pin_ctl.numel(), dtype=torch.uint8, device=self.dev)
            if self.tmp is None or self.tmp.numel() < tmp_bytes:
                self.tmp = torch.empty(_grow(tmp_bytes, 0 if self.tmp is None else self.tmp.numel()), dtype=torch.uint8, device=self.dev)
            grew = True
        if grew:
            self.stats["arena_grows"] += 1

    # ------------------------------------------------------------------ upload
    @_no_grad
    def upload(self, slot: int, items, geoms) -> None:
        import torch
        from . import feed as F
        s = self.slots[slot]
        infos = [self.plan(it, g["h"], g["w"]) for it, g in zip(items, geoms)]
        canvases = {tuple(i["canvas"]) for i in infos}
        if len(canvases) != 1:
            raise ValueError(f"images of one batch letterbox to different canvases: {sorted(canvases)}")
        ch, cw = next(iter(canvases))
        if ch % 32 or cw % 32:
            raise ValueError(f"input size {ch}x{cw} is not a multiple of 32 (letterbox to img_scale first)")
        plans = [i["plan"] for i in infos]
        # images that did not fit the pinned arena when they were decoded: grow it, then place them behind the others
        px_need = s.top
        for g in geoms:
            if g["off"] is None:
                px_need = (px_need + g["h"] * g["w"] * 3 + 255) // 256 * 256
        b = len(items)
        ctl_total, tab_off, elems = F.control_bytes(plans)
        meta_off = ctl_total
        ctl_total += (b * 8 * 4 + 255) // 256 * 256
        tmp_need = sum((p["tmp_bytes"] + 255) // 256 * 256 for p in plans)
        s.ev_up.synchronize()                            # two batches back: long done; orders the host writes below behind it
        self._ensure(s, max(px_need, 256), ctl_total, tmp_need)
        for g in geoms:
            if g["off"] is None:
                n = g["h"] * g["w"] * 3
                g["off"] = s.top
                s.pin_px_np[s.top:s.top + n] = g["spill"].reshape(-1)
                s.top = (s.top + n + 255) // 256 * 256
                g["spill"] = None
        packed = F.pack_batch(plans, [g["off"] for g in geoms], s.pin_ctl_np)
        meta_host = s.pin_ctl_np[meta_off:meta_off + b * 32].view(np.float32).reshape(b, 8)
        meta_host[:] = np.asarray([i["meta"] for i in infos], np.float32)
        px_used = max(s.top, 256)
        tally = dict(launches=0, h2d=0, d2h=0)
        with torch.cuda.stream(self.up_stream):
            self.up_stream.wait_event(s.ev_free)         # the feed kernels of this slot's previous batch have read the arenas
            s.dev_px[:px_used].copy_(s.pin_px[:px_used], non_blocking=True)
            tally["h2d"] += 1
            s.dev_ctl[:ctl_total].copy_(s.pin_ctl[:ctl_total], non_blocking=True)
            tally["h2d"] += 1
            s.ev_up.record(self.up_stream)
        if s.canvas is None or tuple(s.canvas.shape) != (b, ch, cw, 3):
            s.canvas = torch.empty(b, ch, cw, 3, dtype=torch.uint8, device=self.dev)
        meta_dev = s.dev_ctl[meta_off:meta_off + b * 32].view(torch.float32).view(b, 8)
        s.ctx = dict(slot=slot, items=list(items), infos=infos, b=b, hw=(ch, cw), images=packed["images"], tab_off=tab_off, elems=elems,
                     px_used=px_used, meta=meta_dev, tally=tally)
        self.stats["tables_packed"] += packed["n_tables"]

    # ------------------------------------------------------------------ the step
    def _feed(self, s: _Slot) -> None:
        import torch
        from . import feed as F
        c = s.ctx
        main = torch.cuda.current_stream()
        main.wait_event(s.ev_up)
        c["tally"]["launches"] += F.feed_batch_u8(s.dev_px[:c["px_used"]], s.dev_ctl.data_ptr(), c["images"],
                                                  s.dev_ctl.data_ptr() + c["tab_off"], c["elems"], self.tmp, s.canvas)
        s.ev_free.record(main)

    def _tower(self, s: _Slot):
        c = s.ctx
        return self.h.tower(c["b"], c["hw"][0], c["hw"][1])

    @_no_grad
    def issue(self, slot: int) -> None:
        import torch
        from .guarded import layout, typed_views
        s = self.slots[slot]
        c = s.ctx
        self._feed(s)
        tower = self._tower(s)
        self.h.calibrate_first(tower, s.canvas)
        text, counts_dev = self.texts(c)
        res = tower.detect(s.canvas, text, c["meta"], text_counts=counts_dev, overlap_post=True, **self.step_kw())
        # the packed result blob: the step's result tensors + the two range flags
        src = dict({k: res[k] for k in self.RESULT_KEYS}, range_flags=tower.step_range_flags)
        total, lay = layout([(k, t.shape, t.dtype) for k, t in src.items()])
        if s.stage is None or s.stage.numel() < total:
            s.stage = torch.empty(total, dtype=torch.uint8, device=self.dev)
            s.pin_out = torch.empty(total, dtype=torch.uint8).pin_memory()
        post = tower.post_stream
        s.stage.record_stream(post)
        s.stage.record_stream(self.down_stream)
        with torch.cuda.stream(post):                    # the results are produced there, and overwritten by the next step's post
            for k, t in typed_views(s.stage, lay).items():
                t.copy_(src[k], non_blocking=True)
            s.ev_staged.record(post)
        with torch.cuda.stream(self.down_stream):
            self.down_stream.wait_event(s.ev_staged)
            s.pin_out[:total].copy_(s.stage[:total], non_blocking=True)      # ONE packed D2H per batch
            c["tally"]["d2h"] += 1
            s.ev_d2h.record(self.down_stream)
        c["layout"], c["tower"] = lay, tower
        self._tally(c)

    def _tally(self, c: dict) -> None:
        """Folds what was issued for the batch since its last step into the counters."""
        st, t = self.stats, c["tally"]
        st["steps"] += 1
        for k, f in (("feed_launches", "launches"), ("h2d_copies", "h2d"), ("d2h_copies", "d2h")):
            st[k] += t[f]
            st[k + "_max"] = max(st[k + "_max"], t[f])
            t[f] = 0

    @_no_grad
    def collect(self, slot: int):
        from .guarded import tripped, typed_views
        s = self.slots[slot]
        c = s.ctx
        s.ev_d2h.synchronize()
        host = typed_views(s.pin_out, c["layout"])
        tower = c["tower"]
        counts = host["count"].tolist()
        if tripped(counts, [host["range_flags"].tolist()], [tower]):
            return True, []
        return False, [self.result(c, j, host, counts[j], tower) for j in range(c["b"])]

    def inline_only(self) -> bool:
        return self.h.inline_only()

    @_no_grad
    def inline(self, slot: int):
        """The batch through the in-line step (``_TowerHolder.checked_step``), as ``predict`` / ``forward_batch`` run it, from
        the canvas of this slot (written again: a discarded step may not have reached its feed)."""
        s = self.slots[slot]
        c = s.ctx
        self._feed(s)
        tower = self._tower(s)
        tower.clear_range_flags()                        # a discarded later step may have raised them
        text, counts_dev = self.texts(c)
        res, counts = self.h.checked_step(tower, s.canvas, text, c["meta"], text_counts=counts_dev, **self.step_kw())
        host = {}
        for k in self.RESULT_KEYS:
            host[k] = res[k].cpu()
            c["tally"]["d2h"] += 1
        self._tally(c)
        return [self.result(c, j, host, counts[j], tower) for j in range(c["b"])]

    def drain(self) -> None:
        import torch
        torch.cuda.synchronize(self.dev)


def _load_rgb(item, exif: bool) -> np.ndarray:
    """A path (decoded with PIL; ``exif``: orientation applied like cv2.imread, as LoadImageFromFile does), a PIL image or
    an HWC uint8 array -> RGB HWC."""
    if isinstance(item, np.ndarray):
        return item
    from PIL import Image, ImageOps
    if isinstance(item, str):
        with Image.open(item) as im:
            return np.asarray((ImageOps.exif_transpose(im) if exif else im).convert("RGB"))
    if hasattr(item, "convert"):
        return np.asarray(item.convert("RGB"))
    if hasattr(item, "numpy"):
        return item.cpu().numpy()
    raise TypeError(f"cannot decode a {type(item).__name__}")


STREAM_PIPELINE = ("LoadImageFromFile", "WeDetectKeepRatioResize", "WeDetectLetterResize", "LoadAnnotations", "LoadText",
                   "PackDetInputs")


def check_stream_pipeline(pipeline) -> list:
    """The transform objects of ``pipeline`` (a ``Compose``, or the config's list of dicts) if it has the shipped test
    pipeline's shape; raises, naming the transform, on anything else."""
    from .pipeline import Compose
    ts = list(pipeline.transforms) if isinstance(pipeline, Compose) else list(Compose(pipeline).transforms)
    names = [type(t).__name__ for t in ts]
    for i, name in enumerate(names):
        if i >= len(STREAM_PIPELINE) or name != STREAM_PIPELINE[i]:
            raise NotImplementedError(f"the streamed loader runs the shipped test pipeline {list(STREAM_PIPELINE)}; transform "
                                      f"{i} is {name!r} (use the serial loader for other pipelines)")
    if len(names) != len(STREAM_PIPELINE):
        raise NotImplementedError(f"the streamed loader runs the shipped test pipeline; {STREAM_PIPELINE[len(names)]!r} is missing")
    return ts


class MmdetBackend(TowerBackend):
    """``YOLOWorldDetector.predict_stream``: the mmdet test pipeline's geometry (``WeDetectKeepRatioResize`` /
    ``WeDetectLetterResize.geometry``), cv2-family resamples, per-image class banks packed as ``predict`` packs them."""

    def __init__(self, det, pipeline, rescale: bool = True):
        super().__init__(det)
        self.load_t, self.keep, self.letter, _, self.load_text, self.pack = check_stream_pipeline(pipeline)
        self.rescale = rescale

    def load(self, item):
        img = item.get("img")
        if img is not None:                              # already decoded, BGR like LoadImageFromFile's input
            a = img.cpu().numpy() if hasattr(img, "cpu") else np.asarray(img)
            return a[:, :, ::-1]
        return _load_rgb(item["img_path"], True)

    def plan(self, item, h, w):
        from . import feed as F
        from .detector import _meta_of, letterbox_meta
        r = dict(item)
        r.pop("img", None)
        r["img_shape"] = r["ori_shape"] = (h, w)                                    # LoadImageFromFile
        r = self.keep(r)
        g = self.letter.geometry(r, (h, w))
        r = self.load_text(r)
        sample = self.pack.sample(r)
        # the arena holds RGB (what the decoder gives); the serial path flips to BGR, resamples, and flips back in
        # wd_chw_to_hwc_u8 — the resamples are per channel, so writing RGB directly is the same bytes
        p = F.plan_cv(h, w, g["dh"], g["dw"], g["interp"], g["top"], g["left"], g["pad_val"], swap_rb=False)
        hh, ww = g["canvas"]
        return dict(plan=p, canvas=g["canvas"], meta=letterbox_meta(_meta_of(sample), hh, ww, self.rescale), sample=sample)

    def texts(self, c):
        if "text" not in c:
            det = self.det
            banks = [det._bank_for(i["sample"]) for i in c["infos"]]
            cached = {id(v[1]) for v in det._packed_banks.values()}
            packed = det._packed_for(banks, self.dev)
            if packed is None:
                c["tally"]["h2d"] += 0 if banks[0].device == self.dev else 1
                c["text"] = (banks[0].to(self.dev), None)
            else:                                        # a combination packed anew uploads its counts and its host banks
                if id(packed[0]) not in cached:
                    c["tally"]["h2d"] += 1 + sum(1 for t in banks if t.device != self.dev)
                c["text"] = packed
        return c["text"]

    def step_kw(self):
        return dict(self.det._step_kw(), **self.det._best_kw())

    def result(self, c, j, host, n, tower):
        import torch
        from .detector import InstanceData
        s = c["infos"][j]["sample"]
        s.pred_instances = InstanceData(bboxes=host["bboxes"][j, :n].clone(), scores=host["scores"][j, :n].clone(),
                                        labels=host["labels"][j, :n].to(torch.int64))
        return s


class UniBackend(TowerBackend):
    """``SimpleYOLOWorldDetector.predict_stream``: ``letterbox_geometry`` + the Pillow-family resample, proposals with
    embeddings."""

    RESULT_KEYS = ("bboxes", "scores", "labels", "anchors", "count", "embeddings")

    def __init__(self, det, rescale: bool = True, with_embeddings: bool = True):
        super().__init__(det)
        self.rescale = rescale
        if not with_embeddings:
            self.RESULT_KEYS = tuple(k for k in self.RESULT_KEYS if k != "embeddings")

    def load(self, item):
        return _load_rgb(item, False)                    # forward_batch: Image.open(p).convert("RGB")

    def plan(self, item, h, w):
        from . import feed as F
        from .preprocess import letterbox_geometry
        size = self.det.img_size
        nw, nh, left, top, ratio, (dw, dh) = letterbox_geometry(w, h, size)
        if nw < 1 or nh < 1:
            raise ValueError(f"a {w}x{h} image letterboxes to an empty {nw}x{nh} image")
        sc = ratio if self.rescale else 1.0
        return dict(plan=F.plan_pillow(h, w, nh, nw, top, left), canvas=tuple(size), meta=[dw, dh, 0.0, sc, sc, float(w), float(h), 0.0])

    def texts(self, c):
        return self._tower(self.slots[c["slot"]]).P["prompts"], None

    def step_kw(self):
        d = self.det
        return dict(normalize_text=False, score_thr=0.0, with_embed=True, nms="torchvision", nms_param=d.tv_trick_max_numel,
                    nms_device=d.tv_nms_device)

    def result(self, c, j, host, n, tower):
        import torch
        off1, off2 = int(tower.off[1]), int(tower.off[2])
        a = host["anchors"][j, :n].clamp_min(0)
        lvl = (a >= off1).to(torch.int64) + (a >= off2).to(torch.int64)
        out = {"bboxes": host["bboxes"][j, :n].clone(), "scores": host["scores"][j, :n].clone(),
               "labels": host["labels"][j, :n].to(torch.int64),
               "scales": torch.tensor(tower.lvl_logit_scale, dtype=torch.float32)[lvl],
               "bias": torch.tensor(tower.lvl_bias, dtype=torch.float32)[lvl]}
        if "embeddings" in host:
            out["embeddings"] = host["embeddings"][j, :n].clone()
        return out


def predict_stream(backend: TowerBackend, items, batch_size: int, decode_workers: Optional[int] = None, stats: Optional[dict] = None):
    """Generator over the per-image results of ``items``; ``stats`` (a dict, optional) receives the scheduler's and the
    backend's counters when the stream ends."""
    sched = StreamScheduler(backend, batch_size, decode_workers)
    try:
        yield from sched.run(items)
    finally:
        if stats is not None:
            stats.update(backend.stats)
            stats.update(sched.stats)
            stats["decode_workers"] = sched.workers
