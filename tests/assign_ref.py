"""The assignment of include/addons/wedetect_hip_assign.h in numpy: the integer weights (``quant`` / ``weights``), the kernel's
algorithm restated with the same bounded loops (``sap``: shortest augmenting paths with potentials, one private dummy column of
cost 0 per row, the lowest column among equal distances), the independent oracle (``scipy_opt``:
scipy.optimize.linear_sum_assignment) and the uniqueness margin a comparison of PAIRS needs (``uniq_margin``).
``OptRefTracker`` is tests/track_ref.py's tracker with the optimum in place of the greedy picks.  A helper, not a test."""
from __future__ import annotations

import numpy as np
from scipy.optimize import linear_sum_assignment

from tests import track_ref as R

f32 = np.float32
QMAX = 1 << 21
SCALE = float(1 << 20)
STATUS_BOUND, STATUS_BAD = 1, 2          # WD_ASSIGN_STATUS_BOUND / WD_ASSIGN_STATUS_BAD_VALUE


def quant(x) -> np.ndarray:
    """q(x) = (int) min(floorf(x * 2^20), 2^21) for finite x > 0, elementwise in fp32."""
    with np.errstate(over="ignore"):
        y = np.floor(np.asarray(x, f32) * f32(SCALE))
    return np.minimum(y, f32(QMAX)).astype(np.int64)


def weights(val, thr) -> np.ndarray:
    """int64 weights of an fp32 matrix of any shape: q(val) - q(thr) + 1 where val is finite, > 0 and that is >= 1, else 0."""
    val = np.asarray(val, f32)
    good = np.isfinite(val) & (val > 0)
    w = np.where(good, quant(np.where(good, val, f32(1))) - int(quant(f32(thr))) + 1, 0)
    return np.maximum(w, 0).astype(np.int64)


def bad_values(val) -> bool:
    val = np.asarray(val, f32)
    return bool((~np.isfinite(val) | (val < 0)).any())


def sap(W):
    """W int [n_a, n_b] >= 0 (0 = no candidate) -> (match_a list of j or -1, total, steps, bound_hit): the kernel's loops."""
    W = np.asarray(W, np.int64)
    n_a, n_b = W.shape
    INF = np.iinfo(np.int64).max
    u = np.zeros(n_a, np.int64)
    v = np.zeros(n_b + n_a, np.int64)
    col_of = [-1] * n_a
    owner = [-1] * n_b
    cols = np.arange(n_b + n_a)
    steps, bound = 0, False
    for i0 in range(n_a):
        dist = np.full(n_b + n_a, INF)
        used = np.zeros(n_b + n_a, bool)
        prev = np.full(n_b + n_a, -1)
        i, D, sink = i0, 0, -1
        for _ in range(n_a + 1):
            steps += 1
            edge = np.zeros(n_b + n_a, bool)
            edge[:n_b] = W[i] > 0
            edge[n_b + i] = True
            cost = np.zeros(n_b + n_a, np.int64)
            cost[:n_b] = -W[i]
            cur = D + cost - u[i] - v
            better = edge & ~used & (cur < dist)
            dist[better], prev[better] = cur[better], i
            open_ = ~used & (dist != INF)
            if not open_.any():
                break
            c = int(cols[open_][np.argmin(dist[open_])])              # argmin takes the first = the lowest column
            D = int(dist[c])
            used[c] = True
            o = owner[c] if c < n_b else -1
            if o < 0:
                sink = c
                break
            i = o
        if sink < 0:
            bound = True
            continue
        for c in np.nonzero(used[:n_b])[0]:
            d = D - dist[c]
            v[c] -= d
            if owner[c] >= 0:
                u[owner[c]] += d
        u[i0] += D
        c = sink
        for _ in range(n_a + 1):
            r = int(prev[c])
            if c < n_b:
                owner[c] = r
            c, col_of[r] = col_of[r], c
            if r == i0:
                break
    match_a = [c if 0 <= c < n_b else -1 for c in col_of]
    assert np.abs(u).max(initial=0) <= QMAX + 1 and np.abs(v).max(initial=0) <= QMAX + 1 and not v[n_b:].any()   # the int32 bound of the header
    total = int(sum(W[i, j] for i, j in enumerate(match_a) if j >= 0))
    return match_a, total, steps, bound


def scipy_opt(W):
    """-> (sorted list of (i, j) with W > 0 of scipy's maximum-weight assignment, its total)."""
    W = np.asarray(W, np.int64)
    ii, jj = linear_sum_assignment(W, maximize=True)
    pairs = sorted((int(i), int(j)) for i, j in zip(ii, jj) if W[i, j] > 0)
    return pairs, int(sum(W[i, j] for i, j in pairs))


def uniq_margin(W) -> float:
    """optimum - the best optimum with one chosen pair forbidden (re-solved per chosen pair); >= 1 means the optimum is unique:
    another optimal matching would lack one of these pairs (it cannot merely add pairs, each adds weight).  inf without pairs."""
    W = np.asarray(W, np.int64)
    pairs, total = scipy_opt(W)
    m = float("inf")
    for i, j in pairs:
        W2 = W.copy()
        W2[i, j] = 0
        m = min(m, total - scipy_opt(W2)[1])
    return m


def valid_matching(W, match_a, match_b) -> bool:
    """match_a / match_b agree, pair candidates only, use no index twice."""
    n_a, n_b = W.shape
    ma, mb = list(match_a), list(match_b)
    if len(ma) != n_a or len(mb) != n_b:
        return False
    for i, j in enumerate(ma):
        if j >= 0 and not (j < n_b and mb[j] == i and W[i, j] > 0):
            return False
    return all(i < 0 or (i < n_a and ma[i] == j) for j, i in enumerate(mb))


class OptRefTracker(R.RefTracker):
    """RefTracker with the maximum-weight matching as the association of both rounds (wd_track_step_optimal).  Records, per
    association that had a candidate, (uniq_margin / 2^20, pairs taken, IoU-only) in ``assign_calls``; ``assign_margin`` is the
    smallest margin.  The round of a call is told by its rows' scores (round 1: >= high_thr)."""

    def __init__(self, *a, **kw):
        super().__init__(*a, **kw)
        self.assign_calls = []
        self.differs_from_greedy = 0
        self.differs_by_round, self.calls_by_round = [0, 0], [0, 0]             # round 1 / round 2
        self._scores = None

    @property
    def assign_margin(self) -> float:
        return min((c[0] for c in self.assign_calls), default=float("inf"))

    def _frame(self, q, boxes, scores, labels, count, embed):
        self._scores = np.asarray(scores, f32)
        return super()._frame(q, boxes, scores, labels, count, embed)

    def _greedy(self, val, ok, slots, rows, same_slot, same_row):
        if not ok.any():
            return []
        first = bool(self._scores[rows[0]] >= f32(self.p.high_thr))
        thr = self.p.match_thr if first else self.p.iou2_thr
        W = weights(np.where(ok, val, f32(0)), thr)
        pairs, _ = scipy_opt(W)
        if self.margins:
            self.assign_calls.append((uniq_margin(W) / SCALE, len(pairs), (not first) or float(f32(self.p.w_iou)) == 1.0))
            keep, self.margins = self.margins, False
            greedy = super()._greedy(val, ok, slots, rows, same_slot, same_row)
            self.margins = keep
            self.differs_from_greedy += sorted(greedy) != pairs
            self.differs_by_round[0 if first else 1] += sorted(greedy) != pairs
            self.calls_by_round[0 if first else 1] += 1
        return pairs
