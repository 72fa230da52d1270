"""numpy restatement of the top-n result (include/wedetect_hip_topn.h): the n best (score, class) pairs of every row, score
descending, class ascending among equal scores, empty slots (0.0, -1); and a pure-Python model of the key merge the kernels
run (csrc/topn_key.h), one atomic step at a time, for tests/test_cpu_topn.py."""
from __future__ import annotations

import numpy as np

f32 = np.float32


def top_n(scores: np.ndarray, n: int):
    """[R, K] -> (scores [R, n] fp32, labels [R, n] int64): a stable sort by -score keeps the lower class first among equals."""
    scores = np.ascontiguousarray(scores, dtype=f32)
    rows, k = scores.shape
    order = np.argsort(-scores, axis=1, kind="stable")[:, :n]
    s = np.zeros((rows, n), f32)
    lab = np.full((rows, n), -1, np.int64)
    m = min(n, k)
    s[:, :m] = np.take_along_axis(scores, order, axis=1)[:, :m]
    lab[:, :m] = order[:, :m]
    return s, lab


def top_n_loop(scores: np.ndarray, n: int):
    """The same by brute force: n times the maximum of what is left, the first occurrence each time."""
    scores = np.asarray(scores, dtype=f32)
    rows, k = scores.shape
    s = np.zeros((rows, n), f32)
    lab = np.full((rows, n), -1, np.int64)
    for r in range(rows):
        left = list(range(k))
        for j in range(min(n, k)):
            best = left[0]
            for c in left[1:]:
                if scores[r, c] > scores[r, best]:
                    best = c
            s[r, j], lab[r, j] = scores[r, best], best
            left.remove(best)
    return s, lab


# ---- the merge model ---------------------------------------------------------------------------------------------------------
def inserter(slots: list, keys, n: int, stale_bound: bool):
    """A generator that plays ONE producer of csrc/topn_key.h on the shared list ``slots`` (n words of one row): it reads the last
    slot once as its bound (``stale_bound``: at its first step, however long ago that is by the time it offers; otherwise it
    prunes nothing), sorts its keys above the bound in descending order and offers the t-th at slot t — carry = key; old =
    atomic_max(slot[j], carry); carry = min(old, carry) — dropping a carry not above the bound.  Every ``yield`` is a point at which
    the scheduler may run another producer: one between any two memory operations."""
    bound = slots[n - 1] if stale_bound else 0
    yield
    mine = sorted((k for k in keys if k > bound), reverse=True)[:n]
    for t, k in enumerate(mine):
        if stale_bound and t > 0:                # the fused epilogue reads the last slot again between two offers
            bound = max(bound, slots[n - 1])
            yield
        if k <= bound:                           # descending: no later key of this producer is above the bound either
            break
        carry = k
        j = t
        while j < n and carry > bound:
            old = slots[j]                       # atomic max: read-modify-write in one step
            slots[j] = max(old, carry)
            carry = min(old, carry)
            j += 1
            yield


def run_interleaved(producers, rng) -> None:
    """Runs the generators to the end, choosing the next one to step at random."""
    live = list(producers)
    while live:
        g = live[rng.integers(len(live))]
        try:
            next(g)
        except StopIteration:
            live.remove(g)
