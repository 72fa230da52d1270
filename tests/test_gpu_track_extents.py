"""Guard-band tests (GPU) of include/wedetect_hip_track.h, run as tests/test_gpu_exemplar_extents.py runs the entry points of the
exemplar header (the harness of tests/test_gpu_extents.py: its Ctx / Run / Case / execute): every operand is carved from a
tests/arena.py Arena with guard bands, the case runs in 0x00 and in 0xFF surroundings (outputs bit-identical — so every output
element is written — inputs unchanged) and its values are checked once against tests/track_ref.py.

The state and the workspace are carved as workspaces: they start as 0xFF bytes (and, in a third run, as zeros) before
wd_track_reset, and every launch closure starts with the reset, so the harness's second launch on the dirty buffers must repeat the
first one's outputs.  Rows from ``count`` on hold NaN boxes, scores and embeddings: they are never read.

tests/test_cpu_track.py asserts on the CPU that every function of the header that takes device memory has a case here."""
from __future__ import annotations

from typing import List

import numpy as np
import pytest
import torch

import tests.test_gpu_extents as X
import tests.track_hazards  # noqa: F401
from tests import track_cases as TC

pytestmark = pytest.mark.gpu

f32, i32 = torch.float32, torch.int32

CASES: List[X.Case] = []


def case(entry: str, name: str, cap: int = 64 << 20, **kw):
    def deco(fn):
        CASES.append(X.Case(entry, name, (lambda ctx, _fn=fn, _kw=kw: _fn(ctx, **_kw)), cap))
        return fn
    return deco


def _spec(name):
    return [s for s in TC.SPECS if s.name == name][0]


def _operands(ctx, spec):
    from wedetect_amd import track as T
    d = TC.build(spec)
    st = ctx.ws("state", T.state_bytes(spec.n_seq, spec.max_tracks, spec.dim))
    ws = ctx.ws("workspace", T.workspace_bytes(spec.n_seq, spec.max_tracks, spec.max_out))
    inp = dict(boxes=ctx.inp("boxes", torch.from_numpy(d["boxes"]), mis=16), scores=ctx.inp("scores", torch.from_numpy(d["scores"]), mis=4),
               labels=ctx.inp("labels", torch.from_numpy(d["labels"]), mis=4), count=ctx.inp("count", torch.from_numpy(d["count"]), mis=4),
               embed=ctx.inp("embed", torch.from_numpy(d["embed"]), mis=16))
    n_img = spec.n_seq * spec.n_frame
    ids = ctx.out("track_ids", (n_img, spec.max_out), i32, mis=4, fillers=(0,))
    hits = ctx.out("track_hits", (n_img, spec.max_out), i32, mis=4, fillers=(0,))
    params = T.TrackParams(**dict(spec.params)).struct()

    def step():
        T.track_reset(st, spec.n_seq, spec.max_tracks, spec.dim)
        T.track_step(st, ws, inp["boxes"], inp["scores"], inp["labels"], inp["count"], inp["embed"], spec.n_seq, spec.n_frame,
                     spec.max_out, spec.max_tracks, spec.dim, params, ids, hits)
    return st, ids, hits, step


def _export_outs(ctx, spec, vel=True, embed=True):
    n, m = spec.n_seq, spec.max_tracks
    o = dict(ids=ctx.out("ids_out", (n, m), i32, mis=4, fillers=(0,)), labels=ctx.out("labels_out", (n, m), i32, mis=4, fillers=(0,)),
             scores=ctx.out("scores_out", (n, m), mis=4), boxes=ctx.out("boxes_out", (n, m, 4), mis=4), hits=ctx.out("hits", (n, m), i32, mis=4, fillers=(0,)),
             misses=ctx.out("misses", (n, m), i32, mis=4, fillers=(0,)), seq_info=ctx.out("seq_info", (n, 4), i32, mis=4, fillers=(0,)))
    if vel:
        o["vel"] = ctx.out("vel", (n, m, 4), mis=4)
    if embed:
        o["embed"] = ctx.out("embed_out", (n, m, spec.dim), mis=16)
    return o


def _export(T, st, spec, o):
    T.track_export(st, spec.n_seq, spec.max_tracks, spec.dim, o["ids"], o["labels"], o["scores"], o["boxes"], o["hits"], o["misses"],
                   o["seq_info"], o.get("vel"), o.get("embed"))


@case("wd_track_step", "3 sequences x 7 frames of 8 rows, 4 slots, dim 32: overflow, retirement", spec_name="overflow-retire-reuse")
@case("wd_track_step", "1 sequence x 7 frames of 1 row, 4 slots, dim 768: a single row in either round", spec_name="one-row")
@case("wd_track_step", "1 sequence x 7 frames of 65 rows, 64 slots, dim 768: the LDS tile", spec_name="reid-dips-65-rows")
@case("wd_track_step", "1 sequence x 2 frames of 300 rows, 256 slots, dim 768: the matrix in the workspace", spec_name="workspace-300-rows")
def _step(ctx, spec_name):
    spec = _spec(spec_name)
    st, ids, hits, step = _operands(ctx, spec)

    def value(o):
        rids, rhits, _, _ = TC.reference(spec)
        assert np.array_equal(o["track_ids"].cpu().numpy(), rids) and np.array_equal(o["track_hits"].cpu().numpy(), rhits)
    return X.Run(step, lambda: {"track_ids": ids, "track_hits": hits}, value, f"{spec.n_seq} x {spec.n_frame} frames, dim {spec.dim}")


@case("wd_track_export", "3 sequences of 64 slots, dim 768, with velocities and embeddings", spec_name="cameras", vel=True, embed=True)
@case("wd_track_export", "3 sequences of 4 slots, dim 32, neither velocities nor embeddings", spec_name="overflow-retire-reuse", vel=False, embed=False)
def _exp(ctx, spec_name, vel, embed):
    from wedetect_amd import track as T
    spec = _spec(spec_name)
    st, ids, hits, step = _operands(ctx, spec)
    o = _export_outs(ctx, spec, vel, embed)

    def launch():
        step()
        _export(T, st, spec, o)

    def value(got):
        _, _, rex, _ = TC.reference(spec)
        for k in ("ids", "labels", "hits", "misses", "seq_info"):
            assert np.array_equal(got[k].cpu().numpy(), rex[k]), k
        for k in ("scores", "boxes") + (("vel",) if vel else ()):
            assert np.array_equal(got[k].cpu().numpy().view(np.uint32), rex[k].view(np.uint32)), k
        if embed:
            from tests import track_ref as R
            err = np.abs(got["embed"].cpu().numpy().astype(np.float64) - rex["embed"]).max(axis=2)
            assert bool((err <= np.vectorize(lambda u: R.embed_bound(int(u), spec.dim))(rex["n_upd"])).all())
            free = rex["ids"] == 0
            assert not got["embed"].cpu().numpy()[free].any()                 # zero rows for free slots
    return X.Run(launch, lambda: dict(o), value, f"{spec.n_seq} sequences, {spec.max_tracks} slots")


@case("wd_track_reset", "sequences 0 and 2 of 3 reset, sequence 1 kept")
def _reset(ctx):
    """All three sequences run the case, then 0 and 2 are reset: their slots are free and next_id is 1 again; sequence 1 keeps
    what the step left."""
    from wedetect_amd import track as T
    spec = _spec("cameras")
    st, ids, hits, step = _operands(ctx, spec)
    mask = ctx.inp("seq_mask", torch.tensor([1, 0, 7], dtype=i32), mis=4)
    o = _export_outs(ctx, spec, True, False)

    def launch():
        step()
        T.track_reset(st, spec.n_seq, spec.max_tracks, spec.dim, mask)
        _export(T, st, spec, o)

    def value(got):
        _, _, rex, _ = TC.reference(spec)
        info = got["seq_info"].cpu().numpy()
        assert info[0].tolist() == [1, 0, 0, 0] and info[2].tolist() == [1, 0, 0, 0] and info[1].tolist() == rex["seq_info"][1].tolist()
        g = got["ids"].cpu().numpy()
        assert not g[0].any() and not g[2].any() and np.array_equal(g[1], rex["ids"][1]) and g[1].any()
        assert not got["boxes"].cpu().numpy()[[0, 2]].any()
    return X.Run(launch, lambda: dict(o), value, "3 sequences, mask 1 / 0 / 7")


@pytest.mark.parametrize("c", CASES, ids=[c.id for c in CASES])
def test_track_extents(c):
    run0, o0, f0 = X.execute(c, 0x00, 0xFF)
    run1, o1, f1 = X.execute(c, 0xFF, 0xFF)
    X._same(o0, o1, "surroundings 0x00 vs 0xFF")
    _, o2, _ = X.execute(c, 0x00, 0x00)
    X._same(o0, o2, "state and workspace 0xFF vs zero-filled")
    for k, v in o1.items():
        if v.dtype.is_floating_point:
            assert bool(torch.isfinite(v).all()), f"output {k!r}: non-finite elements"
    run0.value(o0)
    print(f"{c.id}: {run0.info}: guards clean, 0x00 == 0xFF, dirty relaunch equal")
