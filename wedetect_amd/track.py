"""ctypes binding of the tracking entry points (include/wedetect_hip_track.h, csrc/track.hip) and ``Tracker``, the object that owns
the state of ``n_seq`` sequences: persistent object ids across the frames of a video, associated on the device from the rows and
region embeddings a detection step keeps.  A version and an export list of its own, like exemplar.py: the main ABI stays as it is."""
from __future__ import annotations

import ctypes as C
import dataclasses
import math
import numbers
from typing import Dict, List, Optional, Sequence

import torch

from . import lib as L
from .lib import i32, i64, vp

TRACK_ABI_VERSION = 1
MAX_TRACKS = 256                 # WD_TRACK_MAX_TRACKS
MAX_OUT = 1024                   # WD_TRACK_MAX_OUT
MAX_DIM = 1024                   # WD_TRACK_MAX_DIM
STATUS_FULL = 1                  # WD_TRACK_STATUS_FULL
STATUS_BAD_COUNT = 2             # WD_TRACK_STATUS_BAD_COUNT
ASSIGNMENTS = ("greedy", "optimal")   # Tracker(assignment=...): wd_track_step / wd_track_step_optimal (wedetect_amd/assign.py)

SIGNATURES = {
    "wd_track_abi_version": (None, []),
    "wd_track_state_bytes": (i64, [i32, i32, i32]),
    "wd_track_workspace_bytes": (i64, [i32, i32, i32]),
    "wd_track_reset": (None, [vp, i32, i32, i32, vp, vp]),
    "wd_track_step": (None, [vp, vp, vp, vp, vp, vp, vp, i32, i32, i32, i32, i32, vp, vp, vp, vp]),
    "wd_track_export": (None, [vp, i32, i32, i32, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp]),
}
EXPORTS = tuple(SIGNATURES)
LIB = L.bind("track", TRACK_ABI_VERSION, SIGNATURES)


class WdTrackParams(C.Structure):
    """struct WdTrackParams of the header, field for field."""
    _fields_ = [("high_thr", C.c_float), ("low_thr", C.c_float), ("new_thr", C.c_float), ("match_thr", C.c_float),
                ("iou2_thr", C.c_float), ("w_iou", C.c_float), ("ema_embed", C.c_float), ("ema_vel", C.c_float),
                ("max_age", C.c_int32), ("match_labels", C.c_int32)]


@dataclasses.dataclass(frozen=True)
class TrackParams:
    """The parameters of the association rule (include/wedetect_hip_track.h).  They are parameters, not tuned values: the defaults
    are the customary starting points of the two-round rule, chosen without any video data."""
    high_thr: float = 0.5
    low_thr: float = 0.1
    new_thr: float = 0.6
    match_thr: float = 0.3
    iou2_thr: float = 0.5
    w_iou: float = 0.5
    ema_embed: float = 0.9
    ema_vel: float = 0.5
    max_age: int = 30
    match_labels: bool = False

    def __post_init__(self):
        for k in ("high_thr", "low_thr", "new_thr", "match_thr", "iou2_thr", "w_iou", "ema_embed", "ema_vel"):
            v = getattr(self, k)
            if isinstance(v, bool) or not isinstance(v, numbers.Real) or not math.isfinite(v):
                raise ValueError(f"TrackParams.{k}: a finite number is expected, got {v!r}")
        if self.low_thr > self.high_thr or self.new_thr < self.high_thr:
            raise ValueError("TrackParams: low_thr <= high_thr <= new_thr is required")
        if not self.match_thr > 0 or not self.iou2_thr > 0:
            raise ValueError("TrackParams: match_thr and iou2_thr must be > 0")
        for k in ("w_iou", "ema_embed", "ema_vel"):
            if not 0.0 <= getattr(self, k) <= 1.0:
                raise ValueError(f"TrackParams.{k} must lie in [0, 1]")
        if isinstance(self.max_age, bool) or not isinstance(self.max_age, numbers.Integral) or self.max_age < 0:
            raise ValueError(f"TrackParams.max_age: an int >= 0 is expected, got {self.max_age!r}")

    def struct(self) -> WdTrackParams:
        return WdTrackParams(self.high_thr, self.low_thr, self.new_thr, self.match_thr, self.iou2_thr, self.w_iou, self.ema_embed,
                             self.ema_vel, int(self.max_age), int(bool(self.match_labels)))


def check_sizes(n_seq, max_tracks, dim) -> None:
    for name, v, lo, hi in (("n_seq", n_seq, 1, 65535), ("max_tracks", max_tracks, 1, MAX_TRACKS), ("dim", dim, 4, MAX_DIM)):
        if isinstance(v, bool) or not isinstance(v, int) or not lo <= v <= hi:
            raise ValueError(f"{name}: an int in {lo}..{hi} is supported, got {v!r}")
    if dim % 4:
        raise ValueError(f"dim: a multiple of 4 is supported, got {dim}")


def state_bytes(n_seq: int, max_tracks: int, dim: int) -> int:
    return int(LIB.wd_track_state_bytes(n_seq, max_tracks, dim))


def workspace_bytes(n_seq: int, max_tracks: int, max_out: int) -> int:
    return int(LIB.wd_track_workspace_bytes(n_seq, max_tracks, max_out))


def track_reset(state, n_seq: int, max_tracks: int, dim: int, seq_mask=None) -> None:
    """``wd_track_reset`` on the current stream: ``state`` uint8 [state_bytes]; ``seq_mask`` int32 [n_seq] or None (all)."""
    L.check(LIB.wd_track_reset(L.ptr(state), int(n_seq), int(max_tracks), int(dim), L.ptr(seq_mask),
                               L.stream_ptr()), "wd_track_reset")


def track_step(state, workspace, boxes, scores, labels, count, embed, n_seq: int, n_frame: int, max_out: int, max_tracks: int,
               dim: int, params: WdTrackParams, track_ids, track_hits) -> None:
    """``wd_track_step`` on the current stream: ``boxes`` fp32 [n_seq * n_frame, max_out, 4], ``scores`` fp32 / ``labels`` int32
    [n_seq * n_frame, max_out], ``count`` int32 [n_seq * n_frame], ``embed`` fp32 [n_seq * n_frame, max_out, dim]; writes
    ``track_ids`` / ``track_hits`` int32 [n_seq * n_frame, max_out], whole, and updates ``state``."""
    L.check(LIB.wd_track_step(L.ptr(state), L.ptr(workspace), L.ptr(boxes), L.ptr(scores), L.ptr(labels), L.ptr(count), L.ptr(embed),
                              int(n_seq), int(n_frame), int(max_out), int(max_tracks), int(dim), C.addressof(params),
                              L.ptr(track_ids), L.ptr(track_hits), L.stream_ptr()), "wd_track_step")


def track_export(state, n_seq: int, max_tracks: int, dim: int, ids, labels, scores, boxes, hits, misses, seq_info, vel=None, embed=None) -> None:
    """``wd_track_export`` on the current stream: int32 [n_seq, max_tracks] ``ids`` / ``labels`` / ``hits`` / ``misses``, fp32
    ``scores`` [n_seq, max_tracks] and ``boxes`` [n_seq, max_tracks, 4], int32 ``seq_info`` [n_seq, 4] (next_id, n_live, status, 0)
    and, if given, fp32 ``vel`` [n_seq, max_tracks, 4] and ``embed`` [n_seq, max_tracks, dim]; every element is written."""
    L.check(LIB.wd_track_export(L.ptr(state), int(n_seq), int(max_tracks), int(dim), L.ptr(ids), L.ptr(labels), L.ptr(scores),
                                L.ptr(boxes), L.ptr(hits), L.ptr(misses), L.ptr(seq_info), L.ptr(vel), L.ptr(embed),
                                L.stream_ptr()), "wd_track_export")


class Tracker:
    """The tracks of ``n_seq`` independent sequences (cameras, videos) on one device: owns the state and the workspace of
    ``wd_track_step``.

        tr = Tracker(1, params=TrackParams(high_thr=0.4))
        res = tower.detect(frames, bank, meta, ..., with_embed=True)      # B consecutive frames of one video
        ids, hits = tr.update(res, n_frame=B)                             # device int32 [B, max_out]; 0 = no track

    ``update`` is one launch on the current stream and never synchronises; the tensors it returns are overwritten by the next
    call."""

    def __init__(self, n_seq: int = 1, max_tracks: int = 128, dim: int = 768, params: Optional[TrackParams] = None, device=None, *,
                 assignment: str = "greedy"):
        check_sizes(n_seq, max_tracks, dim)
        if assignment not in ASSIGNMENTS:
            raise ValueError(f"assignment: one of {ASSIGNMENTS} is expected, got {assignment!r}")
        self.assignment = assignment                      # fixed for the tracker's life
        self._assign = None
        if assignment == "optimal":                       # the add-on binding is loaded only when it is asked for
            from . import assign as _assign
            self._assign = _assign
        self.n_seq, self.max_tracks, self.dim = n_seq, max_tracks, dim
        self.params = params if params is not None else TrackParams()
        if not isinstance(self.params, TrackParams):
            raise TypeError("params must be a track.TrackParams")
        self._struct = self.params.struct()
        dev = torch.device("cuda") if device is None else torch.device(device)
        if dev.type != "cuda":
            raise ValueError(f"Tracker lives on a HIP device, got {device!r}")
        self.device = torch.device("cuda", torch.cuda.current_device() if dev.index is None else dev.index)   # always indexed
        self.state = torch.empty(state_bytes(n_seq, max_tracks, dim), dtype=torch.uint8, device=self.device)
        self._ws: Optional[torch.Tensor] = None
        self._ws_out = 0
        self._out: Dict[tuple, tuple] = {}
        self.reset()

    def reset(self, seqs: Optional[Sequence[int]] = None) -> None:
        """All sequences, or the listed ones, back to "no tracks, next id 1"."""
        mask = None
        if seqs is not None:
            seqs = [int(s) for s in seqs]
            if any(not 0 <= s < self.n_seq for s in seqs):
                raise ValueError(f"reset: sequence indices must lie in 0..{self.n_seq - 1}, got {seqs}")
            host = torch.zeros(self.n_seq, dtype=torch.int32)
            host[seqs] = 1
            mask = host.to(self.device)
        with torch.cuda.device(self.device):
            track_reset(self.state, self.n_seq, self.max_tracks, self.dim, mask)

    def update(self, res: Dict[str, torch.Tensor], n_frame: int = 1):
        """Consumes the result dict of ``ImageTower.detect(..., with_embed=True)`` — ``bboxes`` [B, max_out, 4] in original-image
        pixels, ``scores``, ``labels``, ``count``, ``embeddings`` [B, max_out, dim], on the device — as ``n_seq`` sequences of
        ``n_frame`` consecutive frames (image s * n_frame + f is frame f of sequence s).  Returns device int32 ``track_ids`` and
        ``track_hits`` [B, max_out], aligned with the rows; 0 where a row has no track, and from ``count`` on."""
        if "embeddings" not in res:
            raise ValueError("Tracker.update needs the rows' embeddings: run the step with with_embed=True")
        boxes, scores, labels, count, embed = res["bboxes"], res["scores"], res["labels"], res["count"], res["embeddings"]
        if isinstance(n_frame, bool) or not isinstance(n_frame, int) or n_frame < 1:
            raise ValueError(f"n_frame: a positive int is expected, got {n_frame!r}")
        n_img = self.n_seq * n_frame
        if boxes.dim() != 3 or boxes.shape[0] != n_img or boxes.shape[2] != 4:
            raise ValueError(f"bboxes must be [{n_img} (= n_seq {self.n_seq} x n_frame {n_frame}), max_out, 4], got {tuple(boxes.shape)}")
        max_out = int(boxes.shape[1])
        if not 1 <= max_out <= MAX_OUT:
            raise ValueError(f"max_out: 1..{MAX_OUT} rows per image are supported, got {max_out}")
        for name, t, shape, dt in (("bboxes", boxes, (n_img, max_out, 4), torch.float32), ("scores", scores, (n_img, max_out), torch.float32),
                                   ("labels", labels, (n_img, max_out), torch.int32), ("count", count, (n_img,), torch.int32),
                                   ("embeddings", embed, (n_img, max_out, self.dim), torch.float32)):
            if tuple(t.shape) != shape or t.dtype != dt or t.device != self.device or not t.is_contiguous():
                raise ValueError(f"{name}: a contiguous {dt} tensor {shape} on {self.device} is expected, got {t.dtype} "
                                 f"{tuple(t.shape)} on {t.device}")
        if self._ws is None or max_out > self._ws_out:
            size = workspace_bytes if self._assign is None else self._assign.track_optimal_workspace_bytes
            self._ws = torch.empty(size(self.n_seq, self.max_tracks, max_out), dtype=torch.uint8, device=self.device)
            self._ws_out = max_out
        out = self._out.get((n_img, max_out))
        if out is None:
            self._out.clear()
            out = self._out[(n_img, max_out)] = (torch.empty(n_img, max_out, dtype=torch.int32, device=self.device),
                                                torch.empty(n_img, max_out, dtype=torch.int32, device=self.device))
        step = track_step if self._assign is None else self._assign.track_step_optimal
        with torch.cuda.device(self.device):
            step(self.state, self._ws, boxes, scores, labels, count, embed, self.n_seq, n_frame, max_out, self.max_tracks,
                 self.dim, self._struct, out[0], out[1])
        return out

    def tracks(self, with_embed: bool = False) -> List[dict]:
        """The live tracks of every sequence on the host (one export launch, one synchronising download): per sequence a dict of
        ``ids`` / ``labels`` / ``hits`` / ``misses`` (int32), ``scores``, ``boxes`` / ``velocities`` [n, 4] and ``slots`` of the n live tracks in
        slot order, ``next_id``, ``status`` (bit 0: a track could not start because every slot was taken; bit 1: a frame had a
        negative count) and, with ``with_embed``, ``embeddings`` [n, dim] (zero rows for tracks without one)."""
        n, m, dev = self.n_seq, self.max_tracks, self.device
        ints = torch.empty(4, n, m, dtype=torch.int32, device=dev)
        scores = torch.empty(n, m, dtype=torch.float32, device=dev)
        boxes = torch.empty(n, m, 4, dtype=torch.float32, device=dev)
        info = torch.empty(n, 4, dtype=torch.int32, device=dev)
        vel = torch.empty(n, m, 4, dtype=torch.float32, device=dev)
        emb = torch.empty(n, m, self.dim, dtype=torch.float32, device=dev) if with_embed else None
        with torch.cuda.device(dev):
            track_export(self.state, n, m, self.dim, ints[0], ints[1], scores, boxes, ints[2], ints[3], info, vel, emb)
        ints, scores, boxes, info, vel = ints.cpu(), scores.cpu(), boxes.cpu(), info.cpu(), vel.cpu()
        emb = emb.cpu() if with_embed else None
        out = []
        for s in range(n):
            live = torch.nonzero(ints[0, s] > 0).flatten()
            d = dict(slots=live.to(torch.int32), ids=ints[0, s, live], labels=ints[1, s, live], hits=ints[2, s, live],
                     misses=ints[3, s, live], scores=scores[s, live], boxes=boxes[s, live], velocities=vel[s, live], next_id=int(info[s, 0]),
                     status=int(info[s, 2]))
            assert int(info[s, 1]) == int(live.numel())
            if with_embed:
                d["embeddings"] = emb[s, live]
            out.append(d)
        return out
