"""wd_track_step on the GPU (include/wedetect_hip_track.h) against tests/track_ref.py on the constructed sequences of
tests/track_cases.py: ids, hits, slots, labels, next_id and status equal, boxes and velocities bit-equal, embeddings within
``updates * (dim + 16) * 2^-24`` per component of the reference (elementwise fp32, float64 reductions) — and the three identities:
n_frame frames in one launch == n_frame launches of one frame, a sequence does not depend on the others, two runs give the same
bits.  Every case keeps the margin of track_ref.margin_needed (asserted here and, without a device, in tests/test_cpu_track.py)."""
import numpy as np
import pytest
import torch

import tests.track_hazards  # noqa: F401
from tests import track_cases as TC
from tests import track_ref as R

pytestmark = pytest.mark.gpu

u32 = np.uint32


def _params(spec):
    from wedetect_amd import track as T
    return T.TrackParams(**dict(spec.params))


def run_device(spec, d, per_launch, seqs=None, poison=True):
    """The case on the device in launches of ``per_launch`` frames.  ``seqs``: run only these sequences (as a tracker of
    len(seqs) sequences).  -> (ids, hits, export dict), host arrays."""
    from wedetect_amd import track as T
    seqs = list(range(spec.n_seq)) if seqs is None else seqs
    n_seq, F, mo = len(seqs), spec.n_frame, spec.max_out
    tr = T.Tracker(n_seq, spec.max_tracks, spec.dim, _params(spec))
    if poison:                                                                # the state as it comes: 0xFF bytes, then a reset
        tr.state.fill_(0xFF)
        tr.reset()
    pick = lambda a, f0, f1: np.ascontiguousarray(np.concatenate([a[s * F + f0:s * F + f1] for s in seqs], axis=0))
    ids = np.zeros((n_seq * F, mo), np.int32)
    hits = np.zeros_like(ids)
    for f0 in range(0, F, per_launch):
        f1 = min(f0 + per_launch, F)
        res = dict(bboxes=torch.from_numpy(pick(d["boxes"], f0, f1)).cuda(), scores=torch.from_numpy(pick(d["scores"], f0, f1)).cuda(),
                   labels=torch.from_numpy(pick(d["labels"], f0, f1)).cuda(), count=torch.from_numpy(pick(d["count"], f0, f1)).cuda(),
                   embeddings=torch.from_numpy(pick(d["embed"], f0, f1)).cuda())
        if tr._ws is not None and poison:
            tr._ws.fill_(0xFF)
        ti, th = tr.update(res, f1 - f0)
        ti, th = ti.cpu().numpy().reshape(n_seq, f1 - f0, mo), th.cpu().numpy().reshape(n_seq, f1 - f0, mo)
        for k in range(n_seq):
            ids[k * F + f0:k * F + f1], hits[k * F + f0:k * F + f1] = ti[k], th[k]
    return ids, hits, export(tr)


def export(tr):
    from wedetect_amd import track as T
    n, m = tr.n_seq, tr.max_tracks
    z = lambda *s, dt=torch.int32: torch.full(s, -7, dtype=dt, device="cuda")
    o = dict(ids=z(n, m), labels=z(n, m), scores=z(n, m, dt=torch.float32), boxes=z(n, m, 4, dt=torch.float32), hits=z(n, m),
             misses=z(n, m), seq_info=z(n, 4), vel=z(n, m, 4, dt=torch.float32), embed=z(n, m, tr.dim, dt=torch.float32))
    T.track_export(tr.state, n, m, tr.dim, o["ids"], o["labels"], o["scores"], o["boxes"], o["hits"], o["misses"], o["seq_info"],
                   o["vel"], o["embed"])
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in o.items()}


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(np.ascontiguousarray(a).view(u32), np.ascontiguousarray(b).view(u32))


def assert_equals_reference(spec, ids, hits, ex, rids, rhits, rex, seqs=None):
    seqs = list(range(spec.n_seq)) if seqs is None else seqs
    F = spec.n_frame
    rows = np.concatenate([np.arange(s * F, (s + 1) * F) for s in seqs])
    bad = np.nonzero(ids != rids[rows])
    assert bad[0].size == 0, f"{spec.name}: track ids differ at (image, row) {list(zip(*bad))[:6]}: {ids[bad][:6]} vs {rids[rows][bad][:6]}"
    assert np.array_equal(hits, rhits[rows])
    for k in ("ids", "labels", "hits", "misses", "seq_info"):
        assert np.array_equal(ex[k], rex[k][seqs]), (spec.name, k)
    for k in ("scores", "boxes", "vel"):
        assert same_bits(ex[k], rex[k][seqs]), (spec.name, k)
    err = np.abs(ex["embed"].astype(np.float64) - rex["embed"][seqs].astype(np.float64)).max(axis=2)
    bound = np.vectorize(lambda u: R.embed_bound(int(u), spec.dim))(rex["n_upd"][seqs])
    print(f"{spec.name}: embeddings max |d| {err.max():.3e} (bound of the most updated slot {bound.max():.3e}), "
          f"most updates {int(rex['n_upd'][seqs].max())}")
    assert bool((err <= bound).all()), (spec.name, float(err.max()))
    assert np.isfinite(ex["embed"]).all()


@pytest.mark.parametrize("spec", TC.SPECS, ids=[s.name for s in TC.SPECS])
def test_step_equals_the_reference_and_the_identities_hold(spec):
    d = TC.build(spec)
    rids, rhits, rex, ref = TC.reference(spec)
    print(f"{spec.name}: margin {ref.margin:.3e}, needed {R.margin_needed(spec.dim):.3e}; picks {ref.picks}, exact ties {ref.exact_ties}")
    assert ref.margin >= R.margin_needed(spec.dim)
    ids, hits, ex = run_device(spec, d, spec.n_frame)
    assert_equals_reference(spec, ids, hits, ex, rids, rhits, rex)
    # n_frame frames in one launch == n_frame launches of one frame, bit for bit
    ids1, hits1, ex1 = run_device(spec, d, 1)
    assert np.array_equal(ids, ids1) and np.array_equal(hits, hits1)
    for k in ex:
        assert same_bits(ex[k], ex1[k]), (spec.name, k)
    # two runs give the same bits (the second from a zeroed state and workspace instead of 0xFF bytes)
    ids2, hits2, ex2 = run_device(spec, d, spec.n_frame, poison=False)
    assert np.array_equal(ids, ids2) and np.array_equal(hits, hits2)
    for k in ex:
        assert same_bits(ex[k], ex2[k]), (spec.name, k)
    # a sequence's results do not depend on what the others hold
    if spec.n_seq > 1:
        s = spec.n_seq - 1
        ids3, hits3, ex3 = run_device(spec, d, spec.n_frame, seqs=[s])
        F = spec.n_frame
        assert np.array_equal(ids3, ids[s * F:(s + 1) * F]) and np.array_equal(hits3, hits[s * F:(s + 1) * F])
        for k in ex:
            assert same_bits(ex3[k][0], ex[k][s]), (spec.name, k)


def test_ties_go_to_the_lowest_slot_then_the_lowest_row():
    """Four bit-identical rows, then the same four again: slots 0..3 are born in row order and every later frame matches slot i
    with row i — 16 equal keys but for the slot and row fields."""
    from wedetect_amd import track as T
    dim, mo = 32, 6
    g = np.random.default_rng(3)
    e = g.standard_normal(dim).astype(np.float32)
    boxes = np.tile(np.array([10, 10, 40, 50], np.float32), (3, mo, 1))
    embed = np.tile(e, (3, mo, 1))
    res = dict(bboxes=torch.from_numpy(boxes).cuda(), scores=torch.full((3, mo), 0.9, device="cuda"),
               labels=torch.zeros(3, mo, dtype=torch.int32, device="cuda"), count=torch.tensor([4, 4, 4], dtype=torch.int32, device="cuda"),
               embeddings=torch.from_numpy(embed).cuda())
    tr = T.Tracker(1, 8, dim)
    ids, hits = tr.update(res, 3)
    assert ids.cpu().tolist() == [[1, 2, 3, 4, 0, 0]] * 3 and hits.cpu().tolist() == [[f] * 4 + [0, 0] for f in (1, 2, 3)]
    t = tr.tracks()[0]
    assert t["slots"].tolist() == [0, 1, 2, 3] and t["ids"].tolist() == [1, 2, 3, 4] and t["next_id"] == 5 and t["status"] == 0


def test_reset_of_selected_sequences_and_slot_reuse_lowest_first():
    from wedetect_amd import track as T
    spec = [s for s in TC.SPECS if s.name == "cameras"][0]
    d = TC.build(spec)
    tr = T.Tracker(3, spec.max_tracks, spec.dim)
    res = {k2: torch.from_numpy(d[k]).cuda() for k, k2 in (("boxes", "bboxes"), ("scores", "scores"), ("labels", "labels"),
                                                           ("count", "count"), ("embed", "embeddings"))}
    tr.update(res, spec.n_frame)
    before = tr.tracks()
    tr.reset([1])
    after = tr.tracks()
    assert after[1]["ids"].numel() == 0 and after[1]["next_id"] == 1
    for s in (0, 2):
        assert torch.equal(after[s]["ids"], before[s]["ids"]) and after[s]["next_id"] == before[s]["next_id"] == 31
    ids, _ = tr.update(res, spec.n_frame)
    ids = ids.cpu().numpy().reshape(3, spec.n_frame, -1)
    assert ids[1].max() == 30 and ids[0].max() == 30                          # sequence 1 starts over, the others go on
    with pytest.raises(ValueError):
        tr.reset([3])
