"""Guard-band tests (GPU) of include/addons/wedetect_hip_assign.h, run as tests/test_gpu_track_extents.py runs the entry points of
the tracking header (the harness of tests/test_gpu_extents.py: its Ctx / Run / Case / execute): every operand is carved from a
tests/arena.py Arena with guard bands, the case runs in 0x00 and in 0xFF surroundings (outputs bit-identical — so every output
element is written — inputs unchanged), the workspaces start as 0xFF bytes (and, in a third run, as zeros), and the values are
checked once: wd_assign_max against scipy, wd_track_step_optimal against tests/assign_ref.OptRefTracker.

tests/test_cpu_assign.py asserts on the CPU that every function of the header that takes device memory has a case here."""
from __future__ import annotations

from typing import List

import numpy as np
import pytest
import torch

import tests.test_gpu_extents as X
import tests.track_hazards  # noqa: F401
import tests.assign_hazards  # noqa: F401  (declares the wrappers of wedetect_amd/assign.py to tests/hazards.py)
from tests import assign_ref as A
from tests import track_opt_cases as OC

pytestmark = pytest.mark.gpu

f32, i32, i64 = torch.float32, torch.int32, torch.int64
THR = 0.25

CASES: List[X.Case] = []


def case(entry: str, name: str, cap: int = 64 << 20, **kw):
    def deco(fn):
        CASES.append(X.Case(entry, name, (lambda ctx, _fn=fn, _kw=kw: _fn(ctx, **_kw)), cap))
        return fn
    return deco


@case("wd_assign_max", "3 problems of 65 x 63, a gap of 17 words between them", n_prob=3, n_a=65, n_b=63, gap=17)
@case("wd_assign_max", "1 problem of 7 x 1", n_prob=1, n_a=7, n_b=1, gap=0)
@case("wd_assign_max", "2 problems of 33 x 1024: the widest b-side", n_prob=2, n_a=33, n_b=1024, gap=0)
@case("wd_assign_max", "1 problem of 256 x 40: the full a-side", n_prob=1, n_a=256, n_b=40, gap=0)
def _assign(ctx, n_prob, n_a, n_b, gap):
    from wedetect_amd import assign as WA
    g = np.random.default_rng(n_a * 7 + n_b)
    ld = n_a * n_b + gap
    host = np.full((n_prob, ld), np.nan, np.float32)                           # the gap between problems is never read
    vals = []
    for p in range(n_prob):
        v = g.uniform(THR, 1.0, (n_b, n_a)).astype(np.float32)
        v[g.random((n_b, n_a)) >= 0.6] = 0
        vals.append(v)
        host[p, :n_a * n_b] = v.ravel()
    val = ctx.inp("val", torch.from_numpy(host.ravel()[:(n_prob - 1) * ld + n_a * n_b].copy()), mis=4)
    ma = ctx.out("match_a", (n_prob, n_a), i32, mis=4, fillers=(0,))
    mb = ctx.out("match_b", (n_prob, n_b), i32, mis=4, fillers=(0,))
    total = ctx.out("total", (n_prob,), i64, mis=8, fillers=(0,))
    status = ctx.out("status", (n_prob,), i32, mis=4, fillers=(0,))
    ws = ctx.ws("workspace", WA.workspace_bytes(n_prob, n_a, n_b))

    def launch():
        WA.assign_max_raw(val, n_prob, n_a, n_b, ld, THR, ma, mb, total, status, ws)

    def value(o):
        for p, v in enumerate(vals):
            W = A.weights(v.T, THR)
            pairs, want = A.scipy_opt(W)
            a, b = o["match_a"][p].cpu().tolist(), o["match_b"][p].cpu().tolist()
            assert int(o["total"][p]) == want and int(o["status"][p]) == 0 and A.valid_matching(W, a, b)
            if A.uniq_margin(W) >= 1:
                assert sorted((i, j) for i, j in enumerate(a) if j >= 0) == pairs
    return X.Run(launch, lambda: {"match_a": ma, "match_b": mb, "total": total, "status": status}, value, f"{n_prob} x {n_a} x {n_b}")


def _spec(name):
    return [s for s in OC.SPECS if s.name == name][0]


@case("wd_track_step_optimal", "3 sequences x 7 frames of 8 rows, 4 slots, dim 32: overflow, retirement", spec_name="opt-overflow-retire-reuse")
@case("wd_track_step_optimal", "1 sequence x 7 frames of 1 row, 4 slots, dim 768: a single row in either round", spec_name="opt-one-row")
@case("wd_track_step_optimal", "1 sequence x 7 frames of 65 rows, 64 slots, dim 768: the LDS tile", spec_name="opt-reid-dips-65-rows")
@case("wd_track_step_optimal", "1 sequence x 2 frames of 300 rows, 256 slots, dim 768: the matrix in the workspace", spec_name="opt-workspace-300-rows")
def _step(ctx, spec_name):
    from wedetect_amd import assign as WA
    from wedetect_amd import track as T
    spec = _spec(spec_name)
    d = OC.build(spec)
    st = ctx.ws("state", T.state_bytes(spec.n_seq, spec.max_tracks, spec.dim))
    ws = ctx.ws("workspace", WA.track_optimal_workspace_bytes(spec.n_seq, spec.max_tracks, spec.max_out))
    inp = dict(boxes=ctx.inp("boxes", torch.from_numpy(d["boxes"]), mis=16), scores=ctx.inp("scores", torch.from_numpy(d["scores"]), mis=4),
               labels=ctx.inp("labels", torch.from_numpy(d["labels"]), mis=4), count=ctx.inp("count", torch.from_numpy(d["count"]), mis=4),
               embed=ctx.inp("embed", torch.from_numpy(d["embed"]), mis=16))
    n_img = spec.n_seq * spec.n_frame
    ids = ctx.out("track_ids", (n_img, spec.max_out), i32, mis=4, fillers=(0,))
    hits = ctx.out("track_hits", (n_img, spec.max_out), i32, mis=4, fillers=(0,))
    params = T.TrackParams(**dict(spec.params)).struct()

    def step():
        T.track_reset(st, spec.n_seq, spec.max_tracks, spec.dim)
        WA.track_step_optimal(st, ws, inp["boxes"], inp["scores"], inp["labels"], inp["count"], inp["embed"], spec.n_seq, spec.n_frame,
                              spec.max_out, spec.max_tracks, spec.dim, params, ids, hits)

    def value(o):
        rids, rhits, _, _ = OC.reference(spec)
        assert np.array_equal(o["track_ids"].cpu().numpy(), rids) and np.array_equal(o["track_hits"].cpu().numpy(), rhits)
    return X.Run(step, lambda: {"track_ids": ids, "track_hits": hits}, value, f"{spec.n_seq} x {spec.n_frame} frames, dim {spec.dim}")


@pytest.mark.parametrize("c", CASES, ids=[c.id for c in CASES])
def test_assign_extents(c):
    run0, o0, f0 = X.execute(c, 0x00, 0xFF)
    run1, o1, f1 = X.execute(c, 0xFF, 0xFF)
    X._same(o0, o1, "surroundings 0x00 vs 0xFF")
    _, o2, _ = X.execute(c, 0x00, 0x00)
    X._same(o0, o2, "workspaces 0xFF vs zero-filled")
    run0.value(o0)
    print(f"{c.id}: {run0.info}: guards clean, 0x00 == 0xFF, dirty relaunch equal")
