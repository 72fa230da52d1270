"""The guarded-step protocol of the paths that pipeline tower steps: ``predict_tiled``, ``predict_views`` (detector.py) and
the streamed loader (stream.py).

    1. pipelined pass   every step is issued as ``tower.detect(overlap_post=True)``; its rows are copied into the caller's
                        stacked buffers on the tower's post stream, behind an event of the step
    2. merge + download the caller merges on the device and downloads ONE packed blob (rows, counts, range flags per step)
                        through a pinned twin (``Blob``; parts at 256-byte offsets, ``layout``)
    3. trip             the pipelined steps only DETECT a trip of the fp16x3 range guard (``tripped``): a count of -1, or a
                        raised flag of a tower that is still in fp16x3
    4. in-line pass     after a trip — or while a tower is in its fp32 fallback (``_TowerHolder.inline_only``) — every step runs
                        again in line through ``_TowerHolder.checked_step``, i.e. through ``ImageTower.checked_counts``, which
                        owns the guard's logic (recalibrate, fp32 fallback, the return to fp16x3); the rows are merged again, and
                        a negative count then is an error

``run_steps`` is passes 1-4 for a caller that holds all its steps at once (tiled, views).  The streamed loader's scheduler
decides from outside when a batch is issued, collected or run in line, so it uses the pieces (``layout``, ``tripped``,
``checked_step``, ``inline_only``) and not the driver.  This module launches nothing itself: kernels are the callers'.
"""
from __future__ import annotations

from typing import Callable, Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch

ALIGN = 256


def layout(parts: Sequence[tuple]) -> Tuple[int, List[tuple]]:
    """``[(name, shape, dtype)]`` -> ``(nbytes, [(name, shape, dtype, offset, nbytes)])``: the parts of one packed blob in
    the given order, every offset rounded up to 256 bytes (and so the total).  ``dtype``: a torch or a numpy dtype."""
    off, lay = 0, []
    for name, shape, dt in parts:
        nb = int(np.prod(shape, dtype=np.int64)) * dt.itemsize
        lay.append((name, tuple(shape), dt, off, nb))
        off += (nb + ALIGN - 1) // ALIGN * ALIGN
    return off, lay


def typed_views(blob: torch.Tensor, lay: Sequence[tuple]) -> Dict[str, torch.Tensor]:
    """The parts of ``layout`` as typed views of the uint8 ``blob``, by name."""
    return {name: blob[off:off + nb].view(dt).view(shape) for name, shape, dt, off, nb in lay}


class Blob:
    """One device blob and its pinned twin over ``layout(parts)``: ``dev`` / ``pin`` are the uint8 blobs, ``views`` /
    ``host`` their typed parts by name; ``upload`` / ``fetch`` are the ONE copy in either direction."""

    def __init__(self, parts: Sequence[tuple], device):
        self.nbytes, self.layout = layout(parts)
        self.dev = torch.zeros(self.nbytes, dtype=torch.uint8, device=device)
        self.pin = torch.zeros(self.nbytes, dtype=torch.uint8).pin_memory()
        self.views, self.host = typed_views(self.dev, self.layout), typed_views(self.pin, self.layout)

    def upload(self) -> None:
        self.dev.copy_(self.pin, non_blocking=True)

    def fetch(self) -> Dict[str, torch.Tensor]:
        """Downloads the blob behind the current stream's work, waits for it and returns copies of the host parts."""
        self.pin.copy_(self.dev, non_blocking=True)
        torch.cuda.current_stream().synchronize()
        return {k: t.clone() for k, t in self.host.items()}


def merged_parts(max_out: int, n_steps: int, batch: Tuple[int, ...] = ()) -> tuple:
    """The parts of a merge's staging blob — up to ``max_out`` merged rows (per image of ``batch``), their count, the range
    flags of every step — under the names their device views carry in the caller's buffer dict."""
    f32, i32 = torch.float32, torch.int32
    return (("out_boxes", (*batch, max_out, 4), f32), ("out_scores", (*batch, max_out), f32), ("out_labels", (*batch, max_out), i32),
            ("out_src", (*batch, max_out), i32), ("out_count", batch or (1,), i32), ("flags", (n_steps, 2), i32))


def tripped(counts: Sequence[int], flag_rows: Sequence[Sequence[int]] = (), towers: Sequence = ()) -> bool:
    """Did pipelined steps trip the range guard?  ``counts``: the downloaded counts (only the smallest matters; none = no
    trip); ``flag_rows``: the downloaded range flags, one row per step; ``towers``: the tower of each row — a row counts
    only while its tower's ``precision == "fp16x3"`` (the fp32 kernels never raise a flag, a stale one is not a trip)."""
    return min(counts, default=0) < 0 or any(f for t, row in zip(towers, flag_rows) if t.precision == "fp16x3" for f in row)


def stack_rows(bufs: dict, res: dict, tower, flag_row: int, rows) -> None:
    """Copies a step's rows and its tower's range flags into ``rows`` / ``flag_row`` of the stacked buffers, on the current
    stream."""
    for dst, src in (("boxes", "bboxes"), ("scores", "scores"), ("labels", "labels"), ("counts", "count")):
        bufs[dst][rows].copy_(res[src], non_blocking=True)
    bufs["flags"][flag_row].copy_(tower.step_range_flags, non_blocking=True)


def run_steps(h, steps: Sequence[tuple], kw: dict, bufs: dict, merge_and_download: Callable, stats: Optional[dict]) -> dict:
    """The two-pass driver (module docstring).  ``h``: the ``_TowerHolder``; ``steps``: ``(tower, images, text, text_counts,
    meta, flag_row, rows)`` each — the last two say where ``stack_rows`` puts the step in ``bufs``, the caller's buffer dict:
    stacked ``boxes`` / ``scores`` / ``labels`` / ``counts``, ``flags`` (a part of the downloaded blob), ``events`` (one per
    step); ``kw``: the step keywords; ``merge_and_download()`` -> the host parts of the blob (``merged_parts``); ``stats``:
    a dict whose ``steps`` / ``trips`` / ``inline`` are kept, or None.  Returns the host parts of the pass that counts."""
    stats = {"steps": 0, "trips": 0} if stats is None else stats
    towers = [step[0] for step in steps]
    main = torch.cuda.current_stream()
    inline = h.inline_only()
    if not inline:
        for (tower, x, text, text_counts, meta, *dst), event in zip(steps, bufs["events"]):
            h.calibrate_first(tower, x)
            res = tower.detect(x, text, meta, overlap_post=True, text_counts=text_counts, **kw)
            with torch.cuda.stream(tower.post_stream):       # before the next post-process overwrites the tower's rows
                stack_rows(bufs, res, tower, *dst)
                event.record(tower.post_stream)
        for event in bufs["events"]:
            main.wait_event(event)
        host = merge_and_download()
        stats["steps"] += len(steps)
        if tripped(host["out_count"].tolist(), host["flags"].tolist(), towers):
            inline = True
            stats["trips"] += 1
    if inline:
        torch.cuda.synchronize(h.device)
        for tower in set(towers):
            tower.clear_range_flags()                        # a discarded step may have raised them
        for tower, x, text, text_counts, meta, *dst in steps:
            res, _ = h.checked_step(tower, x, text, meta, text_counts=text_counts, **kw)
            stack_rows(bufs, res, tower, *dst)
        bufs["flags"].zero_()
        host = merge_and_download()
        stats["steps"] += len(steps)
        stats["inline"] = True
        if tripped(host["out_count"].tolist()):
            raise RuntimeError("non-finite scores survived the in-line range guard")
    return host
