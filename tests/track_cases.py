"""Constructed sequences for the tracking tests (tests/test_cpu_track.py checks their margins on the CPU, tests/test_gpu_track_*.py
run them on the device).  A case is a small world of objects: each has a prototype embedding (the prototypes are orthonormal, a
detection's embedding is the prototype plus a little noise at an arbitrary norm) and a box on an integer grid, in cells far enough
apart that different objects never overlap unless the scenario says so.  The scenarios script what a tracker must get right:
objects that vanish and come back elsewhere (re-identification at IoU 0), that stay away past ``max_age`` (retirement, lowest
slot reused), score dips into the second round, label changes, exact duplicates, empty frames and ``count = -1``.

Every case must keep ``track_ref.margin_needed(dim)`` between any evaluated value and its threshold and between a chosen pair and
its competitors — by construction, not by luck: the generators leave the reference alone to decide."""
from __future__ import annotations

import dataclasses
import functools
from typing import Tuple

import numpy as np

from tests import track_ref as R

f32 = np.float32
CELL = 64


@dataclasses.dataclass(frozen=True)
class Spec:
    name: str
    dim: int
    max_tracks: int
    n_obj: int
    n_frame: int
    n_seq: int
    max_out: int
    seed: int = 0
    clutter: int = 0                       # rows below low_thr per frame
    p_vanish: float = 0.0                  # share of objects that leave for ``away`` frames and come back 5000 px away
    away: int = 2
    p_dip: float = 0.0                     # share of (object, frame) with a score in the second round's band
    p_mid: float = 0.0                     # share of objects whose score is >= high_thr but < new_thr: matched, never born
    p_relabel: float = 0.0                 # share of objects whose label changes half way
    dups: int = 0                          # objects that are bit-identical copies of object 0, 1, ...
    spacing: int = CELL                    # distance of the objects' cells; below ~60 the neighbours overlap and compete
    empty: Tuple[int, ...] = ()            # frames with count 0
    bad: Tuple[int, ...] = ()              # frames with count -1
    params: Tuple[Tuple[str, object], ...] = ()

    def ref_params(self) -> R.Params:
        return R.Params(**dict(self.params))


def prototypes(g, dim: int, n: int) -> np.ndarray:
    """n orthonormal rows of ``dim`` elements (n <= dim)."""
    assert n <= dim
    q, _ = np.linalg.qr(g.standard_normal((dim, n)))
    return np.ascontiguousarray(q.T)


def _sequence(spec: Spec, g):
    T, n, mo, dim = spec.n_frame, spec.n_obj, spec.max_out, spec.dim
    p = spec.ref_params()
    proto = prototypes(g, dim, max(n - spec.dups, 1))
    cols = max(int(np.ceil(np.sqrt(max(n, 1) * 4 / 3))), 1)
    pos0 = np.array([[spec.spacing * (k % cols) + 8, spec.spacing * (k // cols) + 8] for k in range(n)], np.int64) + g.integers(0, 4, (n, 2))
    size = g.choice([20, 24, 28], (n, 2))
    vel = g.integers(-2, 3, (n, 2))
    label = g.integers(0, 5, n)
    base = g.uniform(0.65, 0.95, n).astype(f32)
    mid = g.random(n) < spec.p_mid
    base[mid] = g.uniform(p.high_thr + 0.01, p.new_thr - 0.01, int(mid.sum())).astype(f32)
    leave = np.where(g.random(n) < spec.p_vanish, g.integers(1, max(T - spec.away, 2), n), T + 1)
    relabel = np.where(g.random(n) < spec.p_relabel, max(T // 2, 1), T + 1)
    boxes = np.full((T, mo, 4), np.nan, f32)
    scores = np.full((T, mo), np.nan, f32)
    labels = np.full((T, mo), -1, np.int32)
    embed = np.full((T, mo, dim), np.nan, f32)
    count = np.zeros(T, np.int32)
    for f in range(T):
        if f in spec.bad:
            count[f] = -1
            continue
        if f in spec.empty:
            continue
        rows = []
        for k in range(n - spec.dups):
            if leave[k] <= f < leave[k] + spec.away:
                continue
            xy = pos0[k] + vel[k] * f + (5000 if f >= leave[k] + spec.away else 0)
            sc = base[k]
            if g.random() < spec.p_dip and f > 0:
                sc = f32(g.uniform(p.low_thr + 0.05, p.high_thr - 0.05))
            e = proto[k] + 0.02 * g.standard_normal(dim) / np.sqrt(dim)
            e = (e * g.uniform(0.5, 20.0)).astype(f32)
            rows.append((np.array([xy[0], xy[1], xy[0] + size[k, 0], xy[1] + size[k, 1]], f32), f32(sc),
                         int(label[k] + (1 if f >= relabel[k] else 0)), e))
        rows += [rows[d] for d in range(min(spec.dups, len(rows)))]                       # bit-identical copies
        for c in range(spec.clutter):
            e = g.standard_normal(dim).astype(f32)
            xy = g.integers(0, 600, 2)
            rows.append((np.array([xy[0], xy[1], xy[0] + 30, xy[1] + 30], f32), f32(g.uniform(0.0, p.low_thr * 0.9)), 7, e))
        order = g.permutation(len(rows))[:mo]
        count[f] = len(order)
        for r, o in enumerate(order):
            boxes[f, r], scores[f, r], labels[f, r], embed[f, r] = rows[o]
    return boxes, scores, labels, count, embed


@functools.lru_cache(maxsize=None)
def build(spec: Spec):
    """-> dict of the inputs, [n_seq * n_frame, ...]: image s * n_frame + f is frame f of sequence s."""
    g = np.random.default_rng(1000 + spec.seed)
    seqs = [_sequence(spec, g) for _ in range(spec.n_seq)]
    cat = lambda i: np.ascontiguousarray(np.concatenate([s[i] for s in seqs], axis=0))
    return dict(boxes=cat(0), scores=cat(1), labels=cat(2), count=cat(3), embed=cat(4))


@functools.lru_cache(maxsize=None)
def reference(spec: Spec):
    """The reference run of a case, once: (ids, hits, export dict, RefTracker)."""
    d = build(spec)
    ref = R.RefTracker(spec.n_seq, spec.max_tracks, spec.dim, spec.ref_params())
    ids, hits = ref.step(d["boxes"], d["scores"], d["labels"], d["count"], d["embed"], spec.n_frame)
    return ids, hits, ref.export(), ref


P = lambda **kw: tuple(sorted(kw.items()))

SPECS = [
    Spec("one-slot", 32, 1, 2, 2, 1, 4, seed=1),
    Spec("one-row", 768, 4, 1, 7, 1, 1, seed=16, p_dip=0.4),
    Spec("overflow-retire-reuse", 32, 4, 6, 7, 3, 8, seed=2, p_vanish=0.6, away=3, params=P(max_age=1)),
    Spec("reid-dips-65-rows", 768, 64, 56, 7, 1, 65, seed=3, clutter=9, p_vanish=0.3, away=2, p_dip=0.15, p_mid=0.1,
         params=P(max_age=3)),
    Spec("labels-off", 32, 64, 20, 7, 1, 32, seed=4, p_relabel=0.5, p_dip=0.2, clutter=3),
    Spec("labels-on", 32, 64, 20, 7, 1, 32, seed=4, p_relabel=0.5, p_dip=0.2, clutter=3, params=P(match_labels=True)),
    Spec("duplicates", 32, 64, 12, 7, 1, 16, seed=5, dups=4),
    Spec("empty-and-bad-count", 32, 4, 3, 7, 3, 4, seed=6, empty=(0, 3), bad=(5,), params=P(max_age=0)),
    Spec("workspace-300-rows", 768, 256, 300, 2, 1, 300, seed=7),
    Spec("cameras", 768, 64, 30, 2, 3, 40, seed=8, clutter=5),
    Spec("crowd", 32, 64, 16, 7, 1, 16, seed=9, spacing=10, p_dip=0.2, params=P(match_thr=0.17, iou2_thr=0.31)),
]


def crossing(w_iou: float):
    """Two objects with distinct embeddings that cross between frames 2 and 3: frames of 2 rows, row 0 is always object A.
    -> (inputs, params): at the default w_iou the appearance term keeps the ids, at w_iou = 1 the boxes alone swap them."""
    dim, T = 32, 5
    g = np.random.default_rng(42)
    proto = prototypes(g, dim, 2)
    xa, xb = [0, 4, 8, 20, 24], [28, 24, 20, 8, 4]
    boxes, embed = np.zeros((T, 2, 4), f32), np.zeros((T, 2, dim), f32)
    for f in range(T):
        boxes[f, 0], boxes[f, 1] = (xa[f], 0, xa[f] + 24, 24), (xb[f], 0, xb[f] + 24, 24)
        for k in range(2):
            embed[f, k] = ((proto[k] + 0.02 * g.standard_normal(dim) / np.sqrt(dim)) * g.uniform(0.5, 20.0)).astype(f32)
    d = dict(boxes=boxes, scores=np.full((T, 2), 0.9, f32), labels=np.zeros((T, 2), np.int32), count=np.full(T, 2, np.int32), embed=embed)
    return d, R.Params(w_iou=w_iou)
