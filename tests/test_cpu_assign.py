"""The optimal assignment on the CPU: the numpy restatement of the kernel's bounded-loop solver (tests/assign_ref.py) against
scipy.optimize.linear_sum_assignment, the two-by-two example on which greedy and the optimum part ways, the margins of every case
tests/test_gpu_track_optimal.py runs, the add-on header against the binding and the build lists (every check
tests/test_cpu_abi.check_header makes for a public header, made here for include/addons/wedetect_hip_assign.h), the argument
refusals, the host side of the tracker, the detector and the script."""
import ctypes
import os
import re

import numpy as np
import pytest

import tests.assign_hazards  # noqa: F401  (declares the wrappers of wedetect_amd/assign.py to tests/hazards.py)
from tests import assign_ref as A
from tests import track_opt_cases as OC
from tests import track_ref as R
from tests.abi_decl import bound, declared, mismatches

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER_NAME = "addons/wedetect_hip_assign.h"
HEADER = os.path.join(ROOT, "include", "addons", "wedetect_hip_assign.h")
f32 = np.float32
NAMES = ["wd_assign_abi_version", "wd_assign_max", "wd_assign_workspace_bytes", "wd_track_optimal_workspace_bytes", "wd_track_step_optimal"]
SIZE_QUERIES = ("wd_assign_abi_version", "wd_assign_workspace_bytes", "wd_track_optimal_workspace_bytes")


# ------------------------------------------------------------------------------------------------------------ reference
def test_bounded_loop_solver_equals_scipy_on_random_and_tie_heavy_problems():
    g = np.random.default_rng(0)
    shapes = [(1, 1), (1, 9), (9, 1), (40, 60), (60, 40)] + [(int(g.integers(1, 41)), int(g.integers(1, 61))) for _ in range(85)]
    worst, unique = 0.0, 0
    for t, (n_a, n_b) in enumerate(shapes):
        W = g.integers(1, 4, (n_a, n_b)) if t % 3 == 0 else g.integers(1, (1 << 21) + 2, (n_a, n_b))   # ties in {1, 2, 3} / full range
        W = W * (g.random((n_a, n_b)) < (0.1, 0.5, 1.0)[t % 5 % 3])
        match_a, total, steps, hit = A.sap(W)
        pairs, want = A.scipy_opt(W)
        assert total == want and not hit, (t, n_a, n_b)
        mb = [-1] * n_b
        for i, j in enumerate(match_a):
            if j >= 0:
                mb[j] = i
        assert A.valid_matching(W, match_a, mb)
        if A.uniq_margin(W) >= 1:
            unique += 1
            assert sorted((i, j) for i, j in enumerate(match_a) if j >= 0) == pairs, (t, n_a, n_b)
        assert steps <= n_a * (n_a + 1) // 2 + n_a
        worst = max(worst, steps / (n_a * (n_a + 1) / 2 + n_a))
    assert unique >= 30 and worst > 0.5                                        # both kinds occurred; the step bound is not slack


def test_weights_are_the_integer_rule_of_the_header():
    thr = f32(0.3)
    q = lambda x: int(A.quant(f32(x)))
    assert q(1.0) == 1 << 20 and q(2.0) == 1 << 21 and q(5.0) == 1 << 21 and q(3e38) == 1 << 21 and q(1e-30) == 0
    val = np.array([0.0, 0.3, 0.9, np.nan, -0.5, np.inf, 0.1, -0.0], f32)
    w = A.weights(val, thr)
    assert w.tolist() == [0, 1, q(0.9) - q(0.3) + 1, 0, 0, 0, 0, 0] and w.max() <= (1 << 21) + 1
    assert A.bad_values(val) and not A.bad_values(val[[0, 1, 2, 6, 7]])


def test_the_two_by_two_example_greedy_and_optimum_disagree():
    val = np.array([[0.90, 0.89], [0.89, 0.0]], f32)                           # [slot, row]
    ok = val > 0
    never = lambda a, b: False
    g = R.RefTracker(1, 2, 4, margins=False)._greedy(val, ok, np.arange(2), np.arange(2), never, never)
    assert g == [(0, 0)]
    W = A.weights(val, 0.3)
    assert A.scipy_opt(W)[0] == [(0, 1), (1, 0)] and A.sap(W)[0] == [1, 0] and A.uniq_margin(W) >= 1
    # as a sequence: the contested case; and a sequence without competition, on which the two rules agree frame for frame
    d, p = OC.contested()
    args = (d["boxes"], d["scores"], d["labels"], d["count"], d["embed"], 2)
    assert R.RefTracker(1, 4, 32, p).step(*args)[0].tolist() == [[1, 2], [1, 3]]
    opt = A.OptRefTracker(1, 4, 32, p)
    assert opt.step(*args)[0].tolist() == [[1, 2], [2, 1]] and opt.differs_from_greedy == 1
    spec = [s for s in OC.SPECS if s.name == "opt-reid-dips-65-rows"][0]
    dd = OC.build(spec)
    gre, opt = R.RefTracker(1, spec.max_tracks, spec.dim, spec.ref_params()), A.OptRefTracker(1, spec.max_tracks, spec.dim, spec.ref_params())
    for f in range(spec.n_frame):
        one = (dd["boxes"][f:f + 1], dd["scores"][f:f + 1], dd["labels"][f:f + 1], dd["count"][f:f + 1], dd["embed"][f:f + 1], 1)
        (gi, gh), (oi, oh) = gre.step(*one), opt.step(*one)
        assert np.array_equal(gi, oi) and np.array_equal(gh, oh), f
    assert opt.differs_from_greedy == 0 and opt.picks == gre.picks and opt.picks[1] > 10


def _margins_hold(ref, dim):
    """The condition under which the device must give the reference's pairs.  Two matchings differ in total by at most
    2 * (pairs + 1) * (margin_needed(dim) + 2^-20) once each pair's value carries the fp32-tree error and one quantisation step;
    IoU-only associations (w_iou = 1, every round 2) have bit-equal values on the device: a unique optimum suffices."""
    need = R.margin_needed(dim)
    assert ref.thr_margin >= need, ref.thr_margin
    for margin, pairs, iou_only in ref.assign_calls:
        assert margin >= (2.0 ** -20 if iou_only else 2 * (pairs + 1) * (need + 2.0 ** -20)), (margin, pairs, iou_only)


@pytest.mark.parametrize("spec", OC.SPECS, ids=[s.name for s in OC.SPECS])
def test_every_gpu_case_keeps_its_threshold_margin_and_a_unique_optimum(spec):
    ids, hits, ex, ref = OC.reference(spec)
    assert ref.assign_calls and ref.assign_margin < float("inf")
    _margins_hold(ref, spec.dim)
    assert ids.min() >= 0 and ex["seq_info"][:, 2].max() <= 3


def test_the_contested_gpu_case_keeps_its_margins_too():
    d, p = OC.contested()
    ref = A.OptRefTracker(1, OC.CONTESTED_SPEC.max_tracks, OC.CONTESTED_SPEC.dim, p)
    ref.step(d["boxes"], d["scores"], d["labels"], d["count"], d["embed"], 2)
    assert ref.assign_calls == [(ref.assign_margin, 2, True)]
    _margins_hold(ref, OC.CONTESTED_SPEC.dim)
    assert dict(OC.CONTESTED_SPEC.params) == dict(w_iou=p.w_iou, match_thr=p.match_thr)


# ------------------------------------------------------------------------------------------------- header, library, build
def test_header_binding_and_build_lists():
    from wedetect_amd import assign as WA
    from wedetect_amd import build as WB
    from wedetect_amd import lib as L
    from wedetect_amd import track as T
    decl = declared(HEADER_NAME)
    assert sorted(decl) == sorted(WA.EXPORTS) == NAMES and WA.EXPORTS == tuple(WA.SIGNATURES)   # what check_header asserts
    assert not mismatches(decl, WA.SIGNATURES)
    assert not mismatches(decl, bound(WA))
    for name in decl:
        assert hasattr(L.LIB, name)
    assert WA.LIB.wd_assign_abi_version() == WA.ASSIGN_ABI_VERSION == 1
    hdr = open(HEADER).read()
    for macro, val in (("WD_ASSIGN_STATUS_BOUND", WA.STATUS_BOUND), ("WD_ASSIGN_STATUS_BAD_VALUE", WA.STATUS_BAD_VALUE),
                       ("WD_TRACK_STATUS_ASSIGN_BOUND", WA.TRACK_STATUS_ASSIGN_BOUND)):
        assert re.search(rf"#define\s+{macro}\s+{val}\b", hdr), macro
    assert re.search(r"#define\s+WD_ASSIGN_MAX_A\s+WD_TRACK_MAX_TRACKS\b", hdr) and re.search(r"#define\s+WD_ASSIGN_MAX_B\s+WD_TRACK_MAX_OUT\b", hdr)
    assert (WA.MAX_A, WA.MAX_B) == (T.MAX_TRACKS, T.MAX_OUT) and (WA.STATUS_BOUND, WA.STATUS_BAD_VALUE) == (A.STATUS_BOUND, A.STATUS_BAD)
    for name in decl:
        if name in SIZE_QUERIES:
            continue
        doc = hdr[: hdr.index(f"int {name}(")].rsplit("/* ----", 1)[1]
        assert "Extents:" in doc and "WD_ERR_BAD_ARG:" in doc, name
    for name in SIZE_QUERIES[1:]:
        assert getattr(WA.LIB, name).restype is ctypes.c_int64 and re.search(rf"int64_t\s+{name}\(", hdr)
    # wd_track_step_optimal is wd_track_step's arguments in its order, plus workspace_bytes
    step = declared("wedetect_hip_track.h")["wd_track_step"][1]
    assert decl["wd_track_step_optimal"][1] == step[:-1] + ["int64_t workspace_bytes", step[-1]]
    # the build lists
    assert WB.ADDON_HEADERS == [HEADER_NAME] and HEADER_NAME not in WB.PUBLIC_HEADERS and "assign.hip" in WB.SOURCES
    assert os.path.join(ROOT, "include", HEADER_NAME) in WB._headers()
    assert WB.NO_SCRATCH["assign.hip"] == ["assign_max_kernel", "track_step_optimal_kernel"] and WB.ASM_VMEM_SOURCES["assign.hip"] == []
    src = open(os.path.join(WB.CSRC, "assign.hip")).read()
    for k in WB.NO_SCRATCH["assign.hip"]:
        assert re.search(r"__global__[^;{]*\b" + k + r"\(", src), k
    assert "atomic" not in src.replace("no global atomics", "") and "while" not in src       # no atomics; every loop is a bounded for
    # the sizes
    assert WA.workspace_bytes(3, 5, 7) == 48 and WA.workspace_bytes(1, 256, 1024) == 16
    for bad in ((0, 1, 1), (65536, 1, 1), (1, 0, 1), (1, 257, 1), (1, 1, 0), (1, 1, 1025)):
        assert WA.workspace_bytes(*bad) == 0, bad
    assert WA.track_optimal_workspace_bytes(2, 256, 300) == T.workspace_bytes(2, 256, 300) and WA.track_optimal_workspace_bytes(1, 1, 1025) == 0


def test_source_hash_covers_the_addon_header(monkeypatch, tmp_path):
    from wedetect_amd import build as WB
    before = WB.source_hash()
    copy = tmp_path / "include" / "addons"
    copy.mkdir(parents=True)
    for h in WB.PUBLIC_HEADERS:
        (tmp_path / "include" / h).write_bytes(open(os.path.join(ROOT, "include", h), "rb").read())
    (copy / "wedetect_hip_assign.h").write_bytes(open(HEADER, "rb").read() + b"\n")
    monkeypatch.setattr(WB, "ROOT", str(tmp_path))
    assert WB.source_hash() != before                                          # one more byte in the add-on header moves the hash
    (copy / "wedetect_hip_assign.h").write_bytes(open(HEADER, "rb").read())
    assert WB.source_hash() == before


def test_argument_refusals_before_any_launch():
    from wedetect_amd import assign as WA
    from wedetect_amd import track as T
    one, odd, two, four = ctypes.c_void_p(256), ctypes.c_void_p(264), ctypes.c_void_p(258), ctypes.c_void_p(260)
    nan, inf = float("nan"), float("inf")

    def amax(val=one, n_prob=2, n_a=5, n_b=7, ld=35, thr=0.3, ma=one, mb=one, total=one, status=one, ws=one, ws_bytes=32):
        return WA.LIB.wd_assign_max(val, n_prob, n_a, n_b, ld, thr, ma, mb, total, status, ws, ws_bytes, None)

    for kw in (dict(val=None), dict(ma=None), dict(mb=None), dict(total=None), dict(status=None), dict(ws=None), dict(val=two), dict(ma=two),
               dict(mb=two), dict(status=two), dict(total=four), dict(ws=odd), dict(n_prob=0), dict(n_prob=65536), dict(n_a=0), dict(n_a=257),
               dict(n_b=0), dict(n_b=1025), dict(ld=34), dict(ld=-1), dict(ld=2 ** 40), dict(thr=0.0), dict(thr=-0.3), dict(thr=nan), dict(thr=inf)):
        assert amax(**kw) == -1, kw
    assert amax(ws_bytes=31) == -3 and amax(ws_bytes=0) == -3 and amax(n_prob=3, ws_bytes=32) == -3

    good = T.TrackParams().struct()

    def step(state=one, ws=one, boxes=one, scores=one, labels=one, count=one, embed=one, n_seq=2, n_frame=3, max_out=100,
             max_tracks=64, dim=768, params=good, ids=one, hits=one, ws_bytes=2 * 64 * 100 * 4):
        return WA.LIB.wd_track_step_optimal(state, ws, boxes, scores, labels, count, embed, n_seq, n_frame, max_out, max_tracks, dim,
                                            None if params is None else ctypes.addressof(params), ids, hits, ws_bytes, None)

    def bad(**kw):
        d = {f: getattr(good, f) for f, _ in T.WdTrackParams._fields_}
        d.update(kw)
        return T.WdTrackParams(**d)

    # every refusal of wd_track_step (tests/test_cpu_track.py), then the short workspace
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
    assert step(ws_bytes=2 * 64 * 100 * 4 - 1) == -3 and step(ws_bytes=0) == -3


def test_every_assign_entry_point_with_device_memory_has_an_extents_case():
    from tests.test_cpu_arena import _takes_memory
    from tests.test_gpu_assign_extents import CASES
    decl = declared(HEADER_NAME)
    covered = {c.entry for c in CASES}
    for name, params in sorted(decl.items()):
        if name in SIZE_QUERIES:
            assert not _takes_memory(params) and name not in covered
            continue
        assert _takes_memory(params) and name in covered, f"{name}: assign entry without a case in tests/test_gpu_assign_extents.py"
    assert not covered - set(decl)


# ------------------------------------------------------------------------------------------------- tracker, detector, script
def test_tracker_detector_and_script_take_the_assignment_without_a_device():
    import inspect
    import sys
    from wedetect_amd import track as T
    from wedetect_amd.detector import YOLOWorldDetector
    assert T.ASSIGNMENTS == ("greedy", "optimal")
    sig = inspect.signature(T.Tracker.__init__).parameters["assignment"]
    assert sig.default == "greedy" and sig.kind is inspect.Parameter.KEYWORD_ONLY
    for a in ("hungarian", None, 1, "Greedy"):
        with pytest.raises(ValueError, match="assignment"):
            T.Tracker(1, 8, 32, assignment=a)                                  # refused before the device is touched
    d = YOLOWorldDetector("nano")
    with pytest.raises(ValueError, match="assignment"):
        d.track([None] * 2, None, assignment="best")
    with pytest.raises(RuntimeError, match="not on a HIP device"):             # a valid request reaches the device check
        d.track([None] * 2, None, assignment="optimal")
    import infer_wedetect as I
    assert I.parse_args(["--config", "c"]).track_assign == "greedy"
    assert I.parse_args(["--config", "c", "--track", "--track-assign", "optimal"]).track_assign == "optimal"
    for argv in (["--track", "--track-assign", "hungarian"], ["--track-assign", "optimal"]):
        with pytest.raises(SystemExit) as ei:
            I.parse_args(["--config", "c"] + argv)
        assert ei.value.code == 2
    # the binding of the add-on is loaded by the tracker that asks for it, not by wedetect_amd.track
    import ast
    top = [n for n in ast.parse(open(T.__file__).read()).body if isinstance(n, (ast.Import, ast.ImportFrom))]
    assert top and not any("assign" in a.name for n in top for a in n.names)
