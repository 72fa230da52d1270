"""Tracking on the CPU: the numpy restatement (tests/track_ref.py) against its brute-force greedy and hand-made sequences, the
appearance term's point (two crossing objects), the margins of every constructed GPU case, the header against the binding and the
build lists, the argument refusals, the detector's and the script's host side."""
import ctypes
import hashlib
import os
import re

import numpy as np
import pytest

import tests.track_hazards  # noqa: F401  (declares the wrappers of wedetect_amd/track.py to tests/hazards.py)
from tests import track_cases as TC
from tests import track_ref as R
from tests.abi_decl import declared

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "wedetect_hip_track.h")
f32 = np.float32
NAMES = ["wd_track_abi_version", "wd_track_export", "wd_track_reset", "wd_track_state_bytes", "wd_track_step", "wd_track_workspace_bytes"]
SIZE_QUERIES = ("wd_track_abi_version", "wd_track_state_bytes", "wd_track_workspace_bytes")


# ------------------------------------------------------------------------------------------------------------ reference
@pytest.mark.parametrize("spec", TC.SPECS, ids=[s.name for s in TC.SPECS])
def test_every_gpu_case_keeps_its_margin_and_the_sorted_greedy_equals_the_full_scan(spec):
    ids, hits, ex, ref = TC.reference(spec)
    assert ref.margin >= R.margin_needed(spec.dim), (spec.name, ref.thr_margin, ref.pick_margin)
    d = TC.build(spec)
    brute = R.RefTracker(spec.n_seq, spec.max_tracks, spec.dim, spec.ref_params(), brute=True)
    bids, bhits = brute.step(d["boxes"], d["scores"], d["labels"], d["count"], d["embed"], spec.n_frame)
    assert np.array_equal(ids, bids) and np.array_equal(hits, bhits)
    bex = brute.export()
    for k in ex:
        assert np.array_equal(ex[k], bex[k]), k
    # frame by frame in the reference too
    one = R.RefTracker(spec.n_seq, spec.max_tracks, spec.dim, spec.ref_params())
    F = spec.n_frame
    for f in range(F):
        rows = [s * F + f for s in range(spec.n_seq)]
        i1, h1 = one.step(d["boxes"][rows], d["scores"][rows], d["labels"][rows], d["count"][rows], d["embed"][rows], 1)
        assert np.array_equal(i1, ids[rows]) and np.array_equal(h1, hits[rows])
    assert ids.min() >= 0 and bool((ids[d["scores"] != d["scores"]] == 0).all())          # rows from count on carry no id


def test_scenarios_do_what_their_names_say():
    """The reference results the device is held to contain the scenarios: overflow, retirement and reuse of the lowest slot,
    re-identification at IoU 0, second-round matches, exact ties, bad counts."""
    by = {s.name: TC.reference(s) for s in TC.SPECS}
    assert by["overflow-retire-reuse"][2]["seq_info"][:, 2].tolist() == [R.STATUS_FULL] * 3
    assert by["workspace-300-rows"][2]["seq_info"][0].tolist() == [257, 256, R.STATUS_FULL, 0]
    assert by["empty-and-bad-count"][2]["seq_info"][:, 2].tolist() == [R.STATUS_BAD_COUNT] * 3
    assert by["reid-dips-65-rows"][3].picks[1] > 10 and by["crowd"][3].picks[1] > 10          # the second round matched
    assert by["duplicates"][3].exact_ties > 10
    assert by["labels-on"][2]["seq_info"][0, 0] > by["labels-off"][2]["seq_info"][0, 0]          # a changed label starts a new track
    counts = TC.build([s for s in TC.SPECS if s.name == "one-row"][0])["count"]
    assert counts.tolist() == [1] * 7 and by["one-row"][3].picks[0] >= 1 and by["one-row"][3].picks[1] >= 1   # one row per frame, both rounds
    assert by["crowd"][3].pick_margin < 1.0                                                    # competitors existed


def test_greedy_on_random_matrices_with_ties():
    g = np.random.default_rng(0)
    for n_slot, n_row in ((1, 1), (3, 7), (9, 4), (17, 17)):
        val = (g.integers(1, 5, (n_slot, n_row)) / 4).astype(f32)              # few distinct values: ties everywhere
        ok = g.random((n_slot, n_row)) < 0.7
        slots, rows = np.sort(g.choice(64, n_slot, replace=False)), np.sort(g.choice(300, n_row, replace=False))
        never = lambda a, b: False
        a = R.RefTracker(1, 1, 4)._greedy(val, ok, slots, rows, never, never)
        b = R.RefTracker(1, 1, 4, brute=True)._greedy(val, ok, slots, rows, never, never)
        assert a == b and len({i for i, _ in a}) == len(a) == len({j for _, j in a})
        # a loop that knows nothing of keys: best value, then lowest slot, then lowest row
        fi, fj, want = set(range(n_slot)), set(range(n_row)), []
        while True:
            c = [(-val[i, j], i, j) for i in fi for j in fj if ok[i, j]]
            if not c:
                break
            _, i, j = min(c)
            want.append((i, j))
            fi.discard(i)
            fj.discard(j)
        assert a == want
    assert int(R.pack_key(f32(1.0), 2, 5)) == (0x3F800000 << 32) | ((0xFFFF - 2) << 16) | (0xFFFF - 5)


def _frames(rows):
    """rows: per frame a list of (box, score, label, embedding) -> the arrays of one sequence."""
    T, mo, dim = len(rows), max(max(len(r) for r in rows), 1), 4
    boxes, scores = np.zeros((T, mo, 4), f32), np.zeros((T, mo), f32)
    labels, count, embed = np.zeros((T, mo), np.int32), np.zeros(T, np.int32), np.zeros((T, mo, dim), f32)
    for f, fr in enumerate(rows):
        count[f] = len(fr)
        for r, (b, s, l, e) in enumerate(fr):
            boxes[f, r], scores[f, r], labels[f, r], embed[f, r] = b, s, l, e
    return boxes, scores, labels, count, embed


def test_hand_made_sequence():
    ex, ey = [2, 0, 0, 0], [0, 3, 0, 0]
    A = lambda x, s=0.9, l=0, e=ex: ([x, 0, x + 10, 10], s, l, e)
    rows = [[A(0)],                                  # born: id 1, slot 0
            [A(4)],                                  # matched: vel = 0.5 * 0 + 0.5 * 4 = 2
            [A(8, 0.3)],                             # pred 6: round 2 (score below high_thr), IoU 8 / 12; vel = 0.5 * 2 + 0.5 * 4 = 3
            [],                                      # missed: box = pred = 11, misses 1
            [A(500, e=ex), A(14, 0.55, e=ey)],       # re-identified 486 px away by appearance; a 0.55 row never starts a track
            [A(746, 0.7, e=[0, 0, 0, 0])]]           # no usable embedding: sim = 0.5 * iou only, at the predicted place
    ref = R.RefTracker(1, 2, 4, R.Params(max_age=1))
    ids, hits = ref.step(*_frames(rows), 6)
    assert ids[:, 0].tolist() == [1, 1, 1, 0, 1, 1] and hits[:, 0].tolist() == [1, 2, 3, 0, 4, 5] and ids[4, 1] == 0
    q = ref.seqs[0]
    assert q.next_id == 2 and q.status == 0 and q.id.tolist() == [1, 0] and ref.picks == [3, 1]
    # velocities, one rounding per operation: the box of the missed frame is its prediction, 8 + 3 = 11, so the jump of frame 4
    # enters the EMA as 500 - 11 and frame 5 is predicted at 500 + 246
    v4 = f32(f32(0.5) * f32(3)) + f32(f32(0.5) * f32(500 - 11))
    assert v4 == 246 and q.vel[0, 0] == f32(f32(0.5) * v4 + f32(0.5) * f32(746 - 500)) and q.box[0].tolist() == [746, 0, 756, 10]
    assert np.allclose(q.emb[0], [1, 0, 0, 0]) and q.n_upd[0] == 3             # birth + two round-1 updates; round 2 and the zero row add none
    # retirement after max_age and reuse of the lowest slot
    ref = R.RefTracker(1, 2, 4, R.Params(max_age=1))
    rows = [[A(0), A(100, e=ey)], [A(100, e=ey)], [A(100, e=ey)], [A(100, e=ey), A(300, e=[0, 0, 1, 0]), A(400, e=[0, 0, 0, 1])]]
    ids, _ = ref.step(*_frames(rows), 4)
    assert ids.tolist() == [[1, 2, 0], [2, 0, 0], [2, 0, 0], [2, 3, 0]]
    assert ref.seqs[0].id.tolist() == [3, 2] and ref.seqs[0].status == R.STATUS_FULL and ref.seqs[0].next_id == 4
    # count < 0: an empty frame and the status bit; the label rule
    ref = R.RefTracker(1, 2, 4, R.Params(match_labels=True))
    b, s, l, c, e = _frames([[A(0)], [A(0)], [A(0, l=1)]])
    c[1] = -1
    ids, _ = ref.step(b, s, l, c, e, 3)
    assert ids[:, 0].tolist() == [1, 0, 2] and ref.seqs[0].status == R.STATUS_BAD_COUNT and ref.seqs[0].miss.tolist() == [2, 0]


def test_crossing_objects_keep_their_ids_by_appearance_and_swap_them_without():
    """The point of the appearance term.  Row 0 of every frame is object A, row 1 object B."""
    out = {}
    for w in (R.Params().w_iou, 1.0):
        d, p = TC.crossing(w)
        ref = R.RefTracker(1, 8, 32, p)
        ids, _ = ref.step(d["boxes"], d["scores"], d["labels"], d["count"], d["embed"], 5)
        assert ref.margin >= R.margin_needed(32) and ref.seqs[0].next_id == 3
        out[w] = ids[:, :2].tolist()
    assert out[R.Params().w_iou] == [[1, 2]] * 5
    assert out[1.0] == [[1, 2]] * 3 + [[2, 1]] * 2


# ------------------------------------------------------------------------------------------------- header, library, build
def test_library_exports_the_header_and_the_frozen_abi_is_untouched():
    from tests.test_cpu_abi import check_header
    from tests.test_cpu_tile import MAIN_HEADER_SHA256
    from wedetect_amd import lib as L
    from wedetect_amd import track as T
    decl = declared("wedetect_hip_track.h")
    assert sorted(decl) == sorted(T.EXPORTS) == NAMES
    for name in decl:
        assert hasattr(L.LIB, name)
    assert T.LIB.wd_track_abi_version() == T.TRACK_ABI_VERSION == 1
    assert L.LIB.wd_abi_version() == L.ABI_VERSION == 15
    assert hashlib.sha256(open(os.path.join(ROOT, "include", "wedetect_hip.h"), "rb").read()).hexdigest() == MAIN_HEADER_SHA256
    hdr = open(HEADER).read()
    for macro, val in (("WD_TRACK_MAX_TRACKS", T.MAX_TRACKS), ("WD_TRACK_MAX_OUT", T.MAX_OUT), ("WD_TRACK_MAX_DIM", T.MAX_DIM),
                       ("WD_TRACK_STATUS_FULL", T.STATUS_FULL), ("WD_TRACK_STATUS_BAD_COUNT", T.STATUS_BAD_COUNT)):
        assert re.search(rf"#define\s+{macro}\s+{val}\b", hdr), macro
    assert (T.STATUS_FULL, T.STATUS_BAD_COUNT) == (R.STATUS_FULL, R.STATUS_BAD_COUNT)
    conv = {"int32_t": ctypes.c_int32, "float": ctypes.c_float}
    check_header("wedetect_hip_track.h")                                      # argtypes / restype against the prototypes
    for name in decl:
        if name == "wd_track_abi_version":
            continue
        if name in SIZE_QUERIES:
            assert getattr(T.LIB, name).restype is ctypes.c_int64 and re.search(rf"int64_t\s+{name}\(", hdr)
            continue
        doc = hdr[: hdr.index(f"int {name}(")].rsplit("/* ----", 1)[1]
        assert "Extents:" in doc and "WD_ERR_BAD_ARG:" in doc, name
    # struct WdTrackParams, field for field, and the dataclass in front of it
    body = re.search(r"typedef struct WdTrackParams \{(.*?)\} WdTrackParams;", hdr, re.S).group(1)
    fields = re.findall(r"^\s*(float|int32_t)\s+(\w+);", body, re.M)
    assert [(n, conv[t]) for t, n in fields] == list(T.WdTrackParams._fields_)
    assert [n for _, n in fields] == [f.name for f in __import__("dataclasses").fields(T.TrackParams)] == \
        [f.name for f in __import__("dataclasses").fields(R.Params)]
    assert T.TrackParams() == T.TrackParams(**R.Params().__dict__)
    assert "NOT tuned values" in hdr                                          # the header says what the parameters are
    # the sizes
    assert T.state_bytes(1, 128, 768) == 4 * (4 + 14 * 128 + 128 * 768) and T.state_bytes(3, 1, 4) == 3 * 4 * (20 + 4)
    assert T.state_bytes(1, 257, 768) == 0 and T.state_bytes(0, 1, 4) == 0 and T.state_bytes(1, 1, 6) == 0
    assert T.workspace_bytes(2, 256, 300) == 2 * 256 * 300 * 4 and T.workspace_bytes(1, 1, 1) == 16 and T.workspace_bytes(1, 1, 1025) == 0


def test_build_lists_are_as_registered():
    from wedetect_amd import build as WB
    assert "track.hip" in WB.SOURCES and "wedetect_hip_track.h" in WB.PUBLIC_HEADERS
    assert WB.NO_SCRATCH["track.hip"] == ["track_step_kernel", "track_reset_kernel", "track_export_kernel"]
    assert WB.ASM_VMEM_SOURCES["track.hip"] == []
    src = open(os.path.join(WB.CSRC, "track.hip")).read()
    for k in WB.NO_SCRATCH["track.hip"]:
        assert re.search(r"__global__[^;{]*\b" + k + r"\(", src), k
    assert "atomic" not in src.replace("no global atomics", "")               # the selection uses no atomics at all
    entry = open(os.path.join(ROOT, "__graft_entry__.py")).read()
    assert "import wedetect_amd.track " in entry


def test_argument_refusals_before_any_launch():
    from wedetect_amd import track as T
    one, odd, two = ctypes.c_void_p(256), ctypes.c_void_p(264), ctypes.c_void_p(258)
    good = T.TrackParams().struct()

    def step(state=one, ws=one, boxes=one, scores=one, labels=one, count=one, embed=one, n_seq=2, n_frame=3, max_out=100,
             max_tracks=64, dim=768, params=good, ids=one, hits=one):
        return T.LIB.wd_track_step(state, ws, boxes, scores, labels, count, embed, n_seq, n_frame, max_out, max_tracks, dim,
                                   None if params is None else ctypes.addressof(params), ids, hits, None)

    def bad(**kw):
        d = {f: getattr(good, f) for f, _ in T.WdTrackParams._fields_}
        d.update(kw)
        return T.WdTrackParams(**d)

    nan, inf = float("nan"), float("inf")
    for kw in (dict(state=None), dict(ws=None), dict(boxes=None), dict(scores=None), dict(labels=None), dict(count=None),
               dict(embed=None), dict(params=None), dict(ids=None), dict(hits=None), dict(n_seq=0), dict(n_seq=65536), dict(n_frame=0),
               dict(max_out=0), dict(max_out=1025), dict(max_tracks=0), dict(max_tracks=257), dict(dim=0), dict(dim=770), dict(dim=1028),
               dict(state=odd), dict(ws=odd), dict(boxes=odd), dict(embed=odd), dict(scores=two), dict(labels=two), dict(count=two),
               dict(ids=two), dict(hits=two), dict(n_seq=4096, n_frame=64, max_out=1024, dim=1024), dict(n_seq=65535, n_frame=2 ** 31 - 1, max_out=1024, dim=1024),
               dict(n_seq=1, n_frame=2 ** 31 - 1, max_out=1, dim=4),
               dict(params=bad(high_thr=nan)), dict(params=bad(low_thr=inf)), dict(params=bad(low_thr=0.6)), dict(params=bad(new_thr=0.4)),
               dict(params=bad(match_thr=0.0)), dict(params=bad(match_thr=-0.1)), dict(params=bad(iou2_thr=0.0)), dict(params=bad(iou2_thr=nan)),
               dict(params=bad(w_iou=1.5)), dict(params=bad(w_iou=-0.1)), dict(params=bad(ema_embed=2.0)), dict(params=bad(ema_vel=nan)),
               dict(params=bad(max_age=-1))):
        assert step(**kw) == -1, kw

    def reset(state=one, n_seq=2, max_tracks=64, dim=768, mask=None):
        return T.LIB.wd_track_reset(state, n_seq, max_tracks, dim, mask, None)

    for kw in (dict(state=None), dict(state=odd), dict(n_seq=0), dict(max_tracks=300), dict(dim=6), dict(mask=two)):
        assert reset(**kw) == -1, kw

    def export(state=one, n_seq=2, max_tracks=64, dim=768, ids=one, labels=one, scores=one, boxes=one, hits=one, misses=one, info=one,
               vel=None, embed=None):
        return T.LIB.wd_track_export(state, n_seq, max_tracks, dim, ids, labels, scores, boxes, hits, misses, info, vel, embed, None)

    for kw in (dict(state=None), dict(ids=None), dict(labels=None), dict(scores=None), dict(boxes=None), dict(hits=None), dict(misses=None),
               dict(info=None), dict(state=odd), dict(embed=odd), dict(vel=two), dict(ids=two), dict(n_seq=0), dict(max_tracks=0), dict(dim=1028)):
        assert export(**kw) == -1, kw
    # the Python side
    for kw in (dict(high_thr=nan), dict(low_thr=0.7), dict(new_thr=0.3), dict(match_thr=0), dict(iou2_thr=-1), dict(w_iou=1.1),
               dict(ema_embed=-0.5), dict(ema_vel=inf), dict(max_age=-1), dict(max_age=1.5), dict(high_thr="0.5"), dict(high_thr=True)):
        with pytest.raises(ValueError):
            T.TrackParams(**kw)
    for args in ((0, 128, 768), (1, 0, 768), (1, 257, 768), (1, 128, 770), (1, 128, 2048), (True, 128, 768), (1, 128.0, 768)):
        with pytest.raises(ValueError):
            T.check_sizes(*args)
    T.check_sizes(65535, 256, 1024)
    q = T.TrackParams(high_thr=np.float32(0.5), new_thr=np.float64(0.75), max_age=np.int64(3))  # numpy scalars are numbers too
    assert (q.struct().high_thr, q.struct().new_thr, q.struct().max_age) == (0.5, 0.75, 3)


def test_every_track_entry_point_with_device_memory_has_an_extents_case():
    from tests.test_cpu_arena import _takes_memory
    from tests.test_gpu_track_extents import CASES
    decl = declared("wedetect_hip_track.h")
    covered = {c.entry for c in CASES}
    for name, params in sorted(decl.items()):
        if name in SIZE_QUERIES:
            assert not _takes_memory(params) and name not in covered
            continue
        assert _takes_memory(params) and name in covered, f"{name}: track entry without a case in tests/test_gpu_track_extents.py"
    assert not covered - set(decl)
    ids = [c.id for c in CASES]
    assert len(ids) == len(set(ids))


def test_wrappers_are_declared_to_the_happens_before_checker():
    from tests import hazards as H
    assert {"track.track_reset", "track.track_step", "track.track_export"} <= set(H.ACCESS)
    assert not any(w.startswith("track.") for w, _, _ in H.BENIGN)            # plain reads and writes only


# ------------------------------------------------------------------------------------------------- detector and script
def test_detector_refusals_need_no_device():
    from wedetect_amd.detector import YOLOWorldDetector
    d = YOLOWorldDetector("nano")                                             # never moved to a device: the checks come first
    for n_seq in (0, 2, 1.0, True):
        with pytest.raises(ValueError, match="n_seq"):
            d.track([None] * 3, None, n_seq=n_seq)
    with pytest.raises(ValueError, match="track.Tracker"):
        d.track([None] * 2, None, tracker=object())
    with pytest.raises(RuntimeError, match="not on a HIP device"):            # a valid request reaches the device check
        d.track([None] * 2, None, n_seq=2)
    g = YOLOWorldDetector("nano", prompt_groups=True)
    with pytest.raises(NotImplementedError, match="prompt_groups"):
        g.track([None], None)
    d.reset_tracks()
    assert d._tracker is None


def test_script_flags_parse_and_are_off_by_default(capsys):
    import infer_wedetect as I
    a = I.parse_args(["--config", "c"])
    assert a.track is False and a.track_batch == 8 and a.track_high == 0.5 and a.track_max_age == 30
    a = I.parse_args(["--config", "c", "--text", "x", "--image", "frames/", "--track", "--track-batch", "4", "--track-high", "0.4",
                      "--track-low", "0.05", "--track-new", "0.45", "--track-match", "0.2", "--track-iou2", "0.4", "--track-w-iou", "0.7",
                      "--track-max-age", "5", "--track-labels"])
    p = I.track_params(a)
    assert a.track and a.track_batch == 4
    assert (p.high_thr, p.low_thr, p.new_thr, p.match_thr, p.iou2_thr, p.w_iou, p.max_age, p.match_labels) == (0.4, 0.05, 0.45, 0.2, 0.4, 0.7, 5, True)
    for argv, why in ((["--track", "--track-batch", "0"], "--track-batch"), (["--track", "--track-new", "0.3"], "low_thr <= high_thr <= new_thr"),
                      (["--track", "--prompt-groups"], "--prompt-groups"), (["--track-high", "0.4"], "needs --track")):
        with pytest.raises(SystemExit) as ei:
            I.parse_args(["--config", "c"] + argv)
        assert ei.value.code == 2 and why in capsys.readouterr().err
