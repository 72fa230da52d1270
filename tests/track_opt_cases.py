"""The constructed sequences of the optimal-association tests (tests/test_cpu_assign.py checks their margins on the CPU,
tests/test_gpu_track_optimal.py runs them on the device): the generators of tests/track_cases.py with the reference replaced by
tests/assign_ref.OptRefTracker, and ``contested``, the sequence on which the greedy rule and the optimum part ways.

Besides the threshold margin of track_cases every case must have a UNIQUE optimum in every association, by a margin that covers
what the device's fp32 sums may move (tests/test_cpu_assign.py states the condition); the seeds below were picked so that all of
them do.  The ``duplicates`` case of track_cases is not here: bit-identical rows tie exactly, and a tie has no unique optimum."""
from __future__ import annotations

import dataclasses
import functools

import numpy as np

from tests import assign_ref as A
from tests import track_cases as TC
from tests import track_ref as R

f32 = np.float32
Spec, P = TC.Spec, TC.P

SPECS = [
    Spec("opt-one-slot", 32, 1, 2, 2, 1, 4, seed=1),
    Spec("opt-one-row", 768, 4, 1, 7, 1, 1, seed=16, p_dip=0.4),
    Spec("opt-overflow-retire-reuse", 32, 4, 6, 7, 3, 8, seed=2, p_vanish=0.6, away=3, params=P(max_age=1)),
    Spec("opt-reid-dips-65-rows", 768, 64, 56, 7, 1, 65, seed=3, clutter=9, p_vanish=0.3, away=2, p_dip=0.15, p_mid=0.1,
         params=P(max_age=3)),
    Spec("opt-labels-off", 32, 64, 20, 7, 1, 32, seed=4, p_relabel=0.5, p_dip=0.2, clutter=3),
    Spec("opt-labels-on", 32, 64, 20, 7, 1, 32, seed=4, p_relabel=0.5, p_dip=0.2, clutter=3, params=P(match_labels=True)),
    Spec("opt-empty-and-bad-count", 32, 4, 3, 7, 3, 4, seed=6, empty=(0, 3), bad=(5,), params=P(max_age=0)),
    Spec("opt-workspace-300-rows", 768, 256, 300, 2, 1, 300, seed=7),
    Spec("opt-cameras", 768, 64, 30, 2, 3, 40, seed=8, clutter=5),
    Spec("opt-crowd-iou-only", 32, 64, 16, 7, 1, 16, seed=9, spacing=10, p_dip=0.2, params=P(match_thr=0.17, iou2_thr=0.31, w_iou=1.0)),
]

build = TC.build


@functools.lru_cache(maxsize=None)
def reference(spec: Spec):
    """The optimal reference run of a case, once: (ids, hits, export dict, OptRefTracker)."""
    d = build(spec)
    ref = A.OptRefTracker(spec.n_seq, spec.max_tracks, spec.dim, spec.ref_params())
    ids, hits = ref.step(d["boxes"], d["scores"], d["labels"], d["count"], d["embed"], spec.n_frame)
    return ids, hits, ref.export(), ref


def contested():
    """Two objects born side by side, then two rows that contest their two slots (IoU only, w_iou = 1, match_thr = 0.6):

                    row 0 (x = 5)     row 1 (x = -11)
        slot 0      95 / 105          89 / 111
        slot 1      89 / 111          73 / 127 < 0.6: no candidate

    Greedy takes (slot 0, row 0) and leaves slot 1 and row 1 alone: row 1 starts id 3.  The optimum is (slot 0, row 1) and
    (slot 1, row 0): 2 * (89 / 111 - 0.6) > 95 / 105 - 0.6.  -> (inputs of one sequence of 2 frames, params)."""
    dim = 32
    g = np.random.default_rng(7)
    xs = [[0, 16], [5, -11]]
    boxes = np.zeros((2, 2, 4), f32)
    for f in range(2):
        for r in range(2):
            boxes[f, r] = (xs[f][r], 0, xs[f][r] + 100, 10)
    d = dict(boxes=boxes, scores=np.full((2, 2), 0.9, f32), labels=np.zeros((2, 2), np.int32), count=np.full(2, 2, np.int32),
             embed=g.standard_normal((2, 2, dim)).astype(f32))
    return d, R.Params(w_iou=1.0, match_thr=0.6)


CONTESTED_SPEC = dataclasses.replace(SPECS[0], name="opt-contested", max_tracks=4, n_frame=2, max_out=2, params=P(w_iou=1.0, match_thr=0.6))
