"""wd_track_step_optimal on the GPU (include/addons/wedetect_hip_assign.h) against tests/assign_ref.OptRefTracker on the
constructed sequences of tests/track_opt_cases.py, in the comparison form of tests/test_gpu_track_kernels.py: ids, hits, slots,
labels, next_id and status equal, boxes and velocities bit-equal, embeddings within ``embed_bound`` — and the identities: n frames
in one launch == n launches of one frame, a sequence does not depend on the others, two runs give the same bits.  Then the
contested case, where the device must follow the optimum and not the greedy rule, and the detector level.  The margins every case
needs (thresholds, unique optimum) are asserted without a device in tests/test_cpu_assign.py."""
import numpy as np
import pytest
import torch

import tests.assign_hazards  # noqa: F401
import tests.track_hazards  # noqa: F401
from tests import track_opt_cases as OC
from tests import track_ref as R
from tests.test_gpu_track_kernels import assert_equals_reference, export, same_bits

pytestmark = pytest.mark.gpu


def run_device(spec, d, per_launch, seqs=None, poison=True, assignment="optimal"):
    """tests/test_gpu_track_kernels.run_device with the tracker's assignment chosen."""
    from wedetect_amd import track as T
    seqs = list(range(spec.n_seq)) if seqs is None else seqs
    n_seq, F, mo = len(seqs), spec.n_frame, spec.max_out
    tr = T.Tracker(n_seq, spec.max_tracks, spec.dim, T.TrackParams(**dict(spec.params)), assignment=assignment)
    assert tr.assignment == assignment
    if poison:
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


@pytest.mark.parametrize("spec", OC.SPECS, ids=[s.name for s in OC.SPECS])
def test_optimal_step_equals_the_reference_and_the_identities_hold(spec):
    d = OC.build(spec)
    rids, rhits, rex, ref = OC.reference(spec)
    print(f"{spec.name}: threshold margin {ref.thr_margin:.3e}, needed {R.margin_needed(spec.dim):.3e}; uniqueness margin "
          f"{ref.assign_margin:.3e}; picks {ref.picks}, associations that differ from greedy's {ref.differs_from_greedy}")
    ids, hits, ex = run_device(spec, d, spec.n_frame)
    assert_equals_reference(spec, ids, hits, ex, rids, rhits, rex)
    ids1, hits1, ex1 = run_device(spec, d, 1)                                  # n frames in one launch == n launches
    assert np.array_equal(ids, ids1) and np.array_equal(hits, hits1)
    for k in ex:
        assert same_bits(ex[k], ex1[k]), (spec.name, k)
    ids2, hits2, ex2 = run_device(spec, d, spec.n_frame, poison=False)         # two runs, the second from zeroed buffers
    assert np.array_equal(ids, ids2) and np.array_equal(hits, hits2)
    for k in ex:
        assert same_bits(ex[k], ex2[k]), (spec.name, k)
    if spec.n_seq > 1:                                                         # a sequence does not depend on the others
        s = spec.n_seq - 1
        ids3, hits3, ex3 = run_device(spec, d, spec.n_frame, seqs=[s])
        F = spec.n_frame
        assert np.array_equal(ids3, ids[s * F:(s + 1) * F]) and np.array_equal(hits3, hits[s * F:(s + 1) * F])
        for k in ex:
            assert same_bits(ex3[k][0], ex[k][s]), (spec.name, k)


def test_the_contested_case_follows_the_optimum_and_greedy_does_not():
    from tests import assign_ref as A
    d, p = OC.contested()
    spec = OC.CONTESTED_SPEC
    opt = A.OptRefTracker(1, spec.max_tracks, spec.dim, p)
    want, _ = opt.step(d["boxes"], d["scores"], d["labels"], d["count"], d["embed"], 2)
    gre = R.RefTracker(1, spec.max_tracks, spec.dim, p)
    gwant, _ = gre.step(d["boxes"], d["scores"], d["labels"], d["count"], d["embed"], 2)
    assert want.tolist() == [[1, 2], [2, 1]] and gwant.tolist() == [[1, 2], [1, 3]]
    assert opt.assign_margin >= 2.0 ** -20                                     # IoU only: bit-equal values, a unique optimum suffices
    ids, _, ex = run_device(spec, d, 2)
    assert ids.tolist() == want.tolist() and ex["seq_info"][0].tolist() == [3, 2, 0, 0]
    gids, _, gex = run_device(spec, d, 2, assignment="greedy")
    assert gids.tolist() == gwant.tolist() and gex["seq_info"][0].tolist() == [4, 3, 0, 0]


def test_tracker_and_detector_take_the_assignment():
    from wedetect_amd import track as T
    from wedetect_amd.detector import YOLOWorldDetector
    with pytest.raises(ValueError, match="assignment"):
        T.Tracker(1, 8, 32, assignment="hungarian")
    from wedetect_amd import weights as W
    from wedetect_amd.detector import DetDataSample
    from tests.test_gpu_per_image_bank import _stub_encoder
    det = YOLOWorldDetector("nano", test_cfg=dict(max_per_img=50), max_classes=16, text_encoder=_stub_encoder)
    det.load_state_dict({"state_dict": {n: torch.from_numpy(v) for n, v in W.make_state_dict("nano").items()}})
    det.cuda().eval()
    rgb = W.make_images(1, 128, 128, seed=91)[0]
    x = torch.from_numpy(np.ascontiguousarray(rgb[..., ::-1].transpose(2, 0, 1)))
    texts = [f"class {j}" for j in range(5)]
    video = lambda n: ([x] * n, [DetDataSample(metainfo=dict(ori_shape=(128, 128), scale_factor=(1.0, 1.0), texts=texts)) for _ in range(n)])
    params = T.TrackParams(high_thr=0.05, low_thr=0.01, new_thr=0.05)
    plain = [s.pred_instances for s in det.predict(*video(2))]
    out = [s.pred_instances for s in det.track(*video(2), track_params=params, assignment="optimal")]
    assert det._tracker.assignment == "optimal"
    for p, q in zip(plain, out):                                               # every field of predict, bit for bit
        assert torch.equal(p.bboxes.view(torch.int32), q.bboxes.view(torch.int32)) and torch.equal(p.labels, q.labels)
        assert torch.equal(p.scores.view(torch.int32), q.scores.view(torch.int32))
        assert q.track_ids.dtype == torch.int32 and q.track_ids.shape == q.scores.shape == q.track_hits.shape
    ids0 = out[0].track_ids.cpu().numpy()
    born = ids0 > 0
    print(f"nano detector: {len(ids0)} rows, {int(born.sum())} tracks born in the first frame")
    assert born.any()
    again = [s.pred_instances for s in det.track(*video(2), assignment="optimal")]       # a static video: the ids persist over calls
    for f, q in enumerate(out + again):                                        # (rows with one box and embedding tie: as a set)
        assert sorted(q.track_ids.cpu().numpy()[born].tolist()) == sorted(ids0[born].tolist()), f
        assert bool((q.track_hits.cpu().numpy()[born] == f + 1).all()), f
    assert det._tracker.tracks()[0]["next_id"] == int(born.sum()) + 1 and det._tracker.tracks()[0]["status"] == 0
    with pytest.raises(ValueError, match="assignment"):
        det.track(*video(2), assignment="greedy")                              # differs from the kept tracker's
    with pytest.raises(ValueError, match="assignment"):
        det.track(*video(2), tracker=T.Tracker(1, 8, det._tracker.dim, assignment="optimal"), assignment="optimal")
    own = T.Tracker(1, 128, det._tracker.dim, params, assignment="optimal")
    mine = [s.pred_instances for s in det.track(*video(2), tracker=own)]
    assert np.array_equal(mine[0].track_ids.cpu().numpy(), ids0)               # births are in row order under either rule
    det.reset_tracks()
    det.track(*video(1), assignment="greedy")                                  # after a reset the choice is open again
    assert det._tracker.assignment == "greedy"
