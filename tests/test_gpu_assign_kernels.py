"""wd_assign_max on the GPU (include/addons/wedetect_hip_assign.h) against scipy.optimize.linear_sum_assignment through
tests/assign_ref.py: the total always, the pairs wherever the optimum is unique (``uniq_margin >= 1``); tie-heavy matrices
(weights in {1, 2, 3}) are held to the total, to a valid matching and to match_a / match_b agreeing.  Shapes sit where an index or a
reduction bug would show: degenerate sides, rectangular both ways, the wave seam (64 / 65 / 63), the full a-side, the widest
b-side.  The (256, 300) dense case — 256 searches of up to 257 steps — takes well under a second on the device; its scipy side,
uniqueness margin included, takes about as long on the host."""
import numpy as np
import pytest
import torch

import tests.assign_hazards  # noqa: F401  (declares the wrappers of wedetect_amd/assign.py to tests/hazards.py)
from tests import assign_ref as A

pytestmark = pytest.mark.gpu

f32 = np.float32
THR = 0.25
SHAPES = [(1, 1), (1, 7), (7, 1), (5, 3), (3, 5), (64, 64), (65, 63), (256, 300), (33, 1024)]


def random_val(g, n_a, n_b, density=1.0):
    """fp32 [n_b, n_a] in the kernel's layout: candidates uniform in [THR, 1), distinct weights with overwhelming probability."""
    v = g.uniform(THR, 1.0, (n_b, n_a)).astype(f32)
    v[g.random((n_b, n_a)) >= density] = 0
    return v


def tie_val(g, n_a, n_b, density=0.7):
    """weights in {1, 2, 3}: values q steps above the threshold's step."""
    q0 = int(A.quant(f32(THR)))
    w = g.integers(1, 4, (n_b, n_a))
    v = ((q0 + w - 1) * 2.0 ** -20).astype(f32)
    v[g.random((n_b, n_a)) >= density] = 0
    assert np.array_equal(A.weights(v, THR), np.where(v > 0, w, 0))
    return v


def device(vals, thr=THR):
    """A list of [n_b, n_a] problems of one size in one launch -> host (match_a, match_b, total, status)."""
    from wedetect_amd import assign as WA
    out = WA.assign_max(torch.from_numpy(np.ascontiguousarray(np.stack(vals))).cuda(), thr)
    torch.cuda.synchronize()
    return tuple(o.cpu().numpy() for o in out)


def check(val, ma, mb, total, status, unique=None):
    W = A.weights(val.T, THR)                                                  # [n_a, n_b]
    pairs, want = A.scipy_opt(W)
    assert int(total) == want, (val.shape, int(total), want)
    assert A.valid_matching(W, ma.tolist(), mb.tolist())
    assert int(sum(W[i, j] for i, j in enumerate(ma.tolist()) if j >= 0)) == want
    margin = A.uniq_margin(W)
    if unique is not None:
        assert (margin >= 1) == unique, (val.shape, margin)
    if margin >= 1:
        assert sorted((i, j) for i, j in enumerate(ma.tolist()) if j >= 0) == pairs
    assert int(status) == (A.STATUS_BAD if A.bad_values(val) else 0)
    return margin


@pytest.mark.parametrize("n_a,n_b", SHAPES, ids=[f"{a}x{b}" for a, b in SHAPES])
def test_dense_random_problems_equal_scipy_pairs_and_total(n_a, n_b):
    g = np.random.default_rng(n_a * 2000 + n_b)
    val = random_val(g, n_a, n_b)
    ma, mb, total, status = device([val])
    margin = check(val, ma[0], mb[0], total[0], status[0], unique=True)
    print(f"{n_a} x {n_b}: total {int(total[0])}, {int((ma[0] >= 0).sum())} pairs, uniqueness margin {margin:.0f} steps of 2^-20")


@pytest.mark.parametrize("n_a,n_b", [s for s in SHAPES if s != (256, 300)], ids=[f"{a}x{b}" for a, b in SHAPES if (a, b) != (256, 300)])
def test_sparse_and_tie_heavy_problems(n_a, n_b):
    g = np.random.default_rng(n_a * 3000 + n_b)
    sparse = [random_val(g, n_a, n_b, d) for d in (0.1, 0.5)]
    ma, mb, total, status = device(sparse)
    for k, v in enumerate(sparse):
        check(v, ma[k], mb[k], total[k], status[k])
    ties = [tie_val(g, n_a, n_b), tie_val(g, n_a, n_b, 1.0)]                   # marked as such: no pair comparison unless unique
    ma, mb, total, status = device(ties)
    for k, v in enumerate(ties):
        check(v, ma[k], mb[k], total[k], status[k])


def test_empty_full_and_diagonal_problems():
    n = 40
    g = np.random.default_rng(5)
    empty = np.zeros((n, n), f32)
    full = random_val(g, n, n)
    diag = np.zeros((n, n), f32)
    diag[np.arange(n), g.permutation(n)] = g.uniform(THR, 1.0, n).astype(f32)
    ma, mb, total, status = device([empty, full, diag])
    assert (ma[0] == -1).all() and (mb[0] == -1).all() and total[0] == 0 and status[0] == 0
    check(full, ma[1], mb[1], total[1], status[1], unique=True)
    check(diag, ma[2], mb[2], total[2], status[2], unique=True)
    assert (ma[2] >= 0).all() and (mb[2] >= 0).all()


def test_the_two_by_two_example_takes_both_pairs():
    """slot 0: 0.90 / 0.89, slot 1: 0.89 / no candidate — greedy would take (0, 0) alone."""
    val = np.array([[0.90, 0.89], [0.89, 0.0]], f32)                           # val[j][i]
    ma, mb, total, status = device([val], 0.3)
    assert ma[0].tolist() == [1, 0] and mb[0].tolist() == [1, 0] and status[0] == 0
    assert int(total[0]) == 2 * (int(A.quant(f32(0.89))) - int(A.quant(f32(0.3))) + 1)


def test_problems_of_one_launch_are_independent_and_runs_repeat():
    g = np.random.default_rng(11)
    vals = [random_val(g, 65, 63, 0.5), tie_val(g, 65, 63), random_val(g, 65, 63)]
    together = device(vals)
    again = device(vals)
    for a, b in zip(together, again):
        assert np.array_equal(a, b)                                            # two runs, the same bits (ties included)
    for k, v in enumerate(vals):
        alone = device([v])
        for a, b in zip(together, alone):
            assert np.array_equal(a[k], b[0]), k


def test_nan_negative_and_infinite_entries_are_ignored_and_flagged():
    g = np.random.default_rng(13)
    clean = random_val(g, 33, 70, 0.6)
    dirty = clean.copy()
    dirty[3, 5], dirty[10, 0], dirty[69, 32], dirty[20, 20] = np.nan, -0.5, np.inf, -np.inf
    below = clean.copy()
    below[clean > 0] = np.where(g.random(int((clean > 0).sum())) < 0.2, f32(THR / 2), clean[clean > 0])   # positive, below thr: no flag
    ma, mb, total, status = device([clean, dirty, below])
    assert status.tolist() == [0, A.STATUS_BAD, 0]
    for k, v in enumerate((clean, dirty, below)):
        check(v, ma[k], mb[k], total[k], status[k])
    as_zero = np.where(np.isfinite(dirty) & (dirty > 0), dirty, f32(0))
    z = device([as_zero])
    assert np.array_equal(z[0][0], ma[1]) and np.array_equal(z[1][0], mb[1]) and z[2][0] == total[1]
