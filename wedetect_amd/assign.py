"""ctypes binding of the assignment entry points (include/addons/wedetect_hip_assign.h, csrc/assign.hip): the maximum-weight
matching solved on the device — ``assign_max`` on candidate matrices of the caller's, ``track_step_optimal`` as the tracker's
association (``track.Tracker(..., assignment="optimal")`` imports this module; nothing else does).  A version and an export list
of its own, like track.py: the main ABI stays as it is."""
from __future__ import annotations

import ctypes as C
import math

import torch

from . import lib as L
from .lib import f32, i32, i64, vp

ASSIGN_ABI_VERSION = 1
MAX_A = 256                      # WD_ASSIGN_MAX_A
MAX_B = 1024                     # WD_ASSIGN_MAX_B
STATUS_BOUND = 1                 # WD_ASSIGN_STATUS_BOUND
STATUS_BAD_VALUE = 2             # WD_ASSIGN_STATUS_BAD_VALUE
TRACK_STATUS_ASSIGN_BOUND = 4    # WD_TRACK_STATUS_ASSIGN_BOUND

SIGNATURES = {
    "wd_assign_abi_version": (None, []),
    "wd_assign_workspace_bytes": (i64, [i32, i32, i32]),
    "wd_assign_max": (None, [vp, i32, i32, i32, i64, f32, vp, vp, vp, vp, vp, i64, vp]),
    "wd_track_optimal_workspace_bytes": (i64, [i32, i32, i32]),
    "wd_track_step_optimal": (None, [vp, vp, vp, vp, vp, vp, vp, i32, i32, i32, i32, i32, vp, vp, vp, i64, vp]),
}
EXPORTS = tuple(SIGNATURES)
LIB = L.bind("assign", ASSIGN_ABI_VERSION, SIGNATURES)


def workspace_bytes(n_prob: int, n_a: int, n_b: int) -> int:
    return int(LIB.wd_assign_workspace_bytes(n_prob, n_a, n_b))


def track_optimal_workspace_bytes(n_seq: int, max_tracks: int, max_out: int) -> int:
    return int(LIB.wd_track_optimal_workspace_bytes(n_seq, max_tracks, max_out))


def assign_max_raw(val, n_prob: int, n_a: int, n_b: int, ld_prob: int, thr: float, match_a, match_b, total, status, workspace) -> None:
    """``wd_assign_max`` on the current stream, argument for argument."""
    L.check(LIB.wd_assign_max(L.ptr(val), int(n_prob), int(n_a), int(n_b), int(ld_prob), float(thr), L.ptr(match_a), L.ptr(match_b),
                              L.ptr(total), L.ptr(status), L.ptr(workspace), L.nbytes(workspace), L.stream_ptr()), "wd_assign_max")


def assign_max(val: torch.Tensor, thr: float, workspace=None):
    """The maximum-weight matching of every problem of ``val``, fp32 [n_prob, n_b, n_a] or [n_b, n_a] on the device, contiguous:
    ``val[p, j, i]`` is the value of slot-side index i with row-side index j, 0 = no candidate, a candidate is >= ``thr`` > 0
    (the header's result definition: integer weights, exact optimum).  Returns device tensors ``match_a`` int32 [n_prob, n_a] (the
    j of i, or -1), ``match_b`` int32 [n_prob, n_b], ``total`` int64 [n_prob] and ``status`` int32 [n_prob] (bit 1: a negative
    or non-finite value was ignored) — without the leading dimension for a 2-d ``val``.  One launch, no synchronisation."""
    if not isinstance(val, torch.Tensor) or val.dtype != torch.float32 or val.device.type != "cuda" or not val.is_contiguous():
        raise ValueError("assign_max: a contiguous fp32 tensor on a HIP device is expected")
    if val.dim() not in (2, 3):
        raise ValueError(f"assign_max: val must be [n_prob, n_b, n_a] or [n_b, n_a], got {tuple(val.shape)}")
    if isinstance(thr, bool) or not math.isfinite(thr) or not thr > 0:
        raise ValueError(f"assign_max: thr must be finite and > 0, got {thr!r}")
    v3 = val if val.dim() == 3 else val[None]
    n_prob, n_b, n_a = (int(x) for x in v3.shape)
    if not (1 <= n_prob <= 65535 and 1 <= n_a <= MAX_A and 1 <= n_b <= MAX_B):
        raise ValueError(f"assign_max: 1..65535 problems of 1..{MAX_A} x 1..{MAX_B} are supported, got {n_prob} of {n_a} x {n_b}")
    dev = val.device
    need = workspace_bytes(n_prob, n_a, n_b)
    if workspace is None:
        workspace = torch.empty(need, dtype=torch.uint8, device=dev)
    match_a = torch.empty(n_prob, n_a, dtype=torch.int32, device=dev)
    match_b = torch.empty(n_prob, n_b, dtype=torch.int32, device=dev)
    total = torch.empty(n_prob, dtype=torch.int64, device=dev)
    status = torch.empty(n_prob, dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        assign_max_raw(v3, n_prob, n_a, n_b, n_a * n_b, thr, match_a, match_b, total, status, workspace)
    if val.dim() == 2:
        return match_a[0], match_b[0], total[0], status[0]
    return match_a, match_b, total, status


def track_step_optimal(state, workspace, boxes, scores, labels, count, embed, n_seq: int, n_frame: int, max_out: int, max_tracks: int,
                       dim: int, params, track_ids, track_hits) -> None:
    """``wd_track_step_optimal`` on the current stream: ``track.track_step``'s arguments and results, the association of rounds 1
    and 2 being the maximum-weight matching; ``workspace`` is sized by ``track_optimal_workspace_bytes``."""
    L.check(LIB.wd_track_step_optimal(L.ptr(state), L.ptr(workspace), L.ptr(boxes), L.ptr(scores), L.ptr(labels), L.ptr(count),
                                      L.ptr(embed), int(n_seq), int(n_frame), int(max_out), int(max_tracks), int(dim),
                                      C.addressof(params), L.ptr(track_ids), L.ptr(track_hits), L.nbytes(workspace), L.stream_ptr()),
            "wd_track_step_optimal")
