"""Single-label ("best class") detection on the CPU: the numpy restatement of the reference's multi_label=False branch
(tests/best_ref.py) against the fixture the reference's own functions wrote (tests/golden/best_class.npz), the 64-bit key,
the public switches and the refusals that stay, the header against the binding."""
import os
import re

import numpy as np
import pytest

import tests.best_hazards  # noqa: F401  (declares the wrappers of wedetect_amd/best.py to tests/hazards.py)
from oracle import postprocess as opp
from tests import best_ref as R
from tests.util import golden

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _levels_to_scores(q):
    return ((q.astype(np.float32) + np.float32(1)) / np.float32(4096)).astype(np.float32)


def test_best_ref_reproduces_the_reference_fixture_exactly():
    fx = golden("best_class.npz")
    q = fx["levels"]
    assert q.shape == (2, 525, 300) and q.dtype == np.uint16
    thr, nms_pre = float(fx["score_thr"]), int(fx["nms_pre"])
    ties = 0
    for b in range(2):
        s, lab, anc = R.candidates(_levels_to_scores(q[b]), thr, nms_pre)
        assert np.array_equal(s, fx[f"img{b}.scores"]) and s.dtype == np.float32
        assert np.array_equal(lab, fx[f"img{b}.labels"]) and np.array_equal(anc, fx[f"img{b}.anchors"])
        assert s.shape[0] == nms_pre and int((R.best_class(_levels_to_scores(q[b]))[0] > np.float32(thr)).sum()) > nms_pre    # cut inside the list
        ties += int((np.diff(s) == 0).sum())
    assert ties > 0                                              # equal scores in the top-k: the anchor breaks them
    # the planted rows: three classes tie -> the lowest; a constant row -> class 0; class 0 and the last class
    sc0 = _levels_to_scores(q[0])
    best, lab = R.best_class(sc0)
    assert lab[10] == 7 and lab[11] == 0 and lab[200] == 0 and lab[201] == 299 and best[200] == best[201]
    a0 = fx["img0.anchors"].tolist()
    assert a0.index(200) + 1 == a0.index(201)                    # equal scores: anchor ascending
    top = fx["img1.scores"] == np.float32(1.0)                   # the rows that tie at the largest score: anchor ascending
    a1, l1 = fx["img1.anchors"][top].tolist(), fx["img1.labels"][top].tolist()
    assert a1 == sorted(a1) and a1[0] == 3 and a1[-1] == 524 and (l1[0], l1[-1]) == (298, 1) and bool(top[: len(a1)].all())


def test_key_round_trip_and_tie_rule():
    from wedetect_amd import best as BS
    g = np.random.default_rng(5)
    s = g.random(4096, dtype=np.float32)
    s[:4] = (0.0, 1.0, np.float32(1e-45), 0.5)                   # +0, the largest score, a denormal
    c = g.integers(0, 2 ** 31 - 1, 4096)
    c[:3] = (0, 2 ** 31 - 2, 1 << 20)
    key = BS.pack_key(s.view(np.uint32), c)
    assert key.dtype == np.uint64 and bool((key != 0).all())    # no valid (score, class) packs to "no class seen"
    s2, c2 = BS.unpack_key(key)
    assert np.array_equal(s2.view(np.uint32), s.view(np.uint32)) and np.array_equal(c2, c.astype(np.int32))
    assert [v.tolist() for v in BS.unpack_key(np.zeros(2, np.uint64))] == [[0.0, 0.0], [-1, -1]]
    # the unsigned order of the keys: score first, then the LOWER class
    order = np.lexsort((-c, s.view(np.uint32)))
    assert np.array_equal(np.argsort(key, kind="stable"), order)
    # max over a row's keys = numpy's max / argmax (first occurrence), ties included
    rows = (np.round(g.random((64, 300), dtype=np.float32) * 8) / 8).astype(np.float32)
    keys = BS.pack_key(rows.view(np.uint32), np.arange(300)[None, :] + 1000)
    bs, bl = BS.unpack_key(keys.max(axis=1))
    best, lab = R.best_class(rows)
    assert np.array_equal(bs, best) and np.array_equal(bl, lab + 1000)
    assert int((rows == best[:, None]).sum(1).max()) > 1       # rows with several maxima were seen
    # merging chunks in any order is one maximum
    parts = [BS.pack_key(rows[:, a:b].view(np.uint32), np.arange(a, b)[None, :]).max(axis=1) for a, b in ((200, 300), (0, 120), (120, 200))]
    assert np.array_equal(BS.unpack_key(np.maximum.reduce(parts))[1], lab)


def test_best_ref_nms_forms_on_hand_made_boxes():
    bx = np.asarray([[0, 0, 10, 10], [1, 1, 11, 11], [50, 50, 60, 60], [0, 0, 10, 10]], np.float32)
    sc = np.asarray([0.9, 0.8, 0.7, 0.6], np.float32)
    lb = np.asarray([0, 1, 1, 0], np.int64)
    meta = [0, 0, 0, 1, 1, 100, 100, 1]
    aware = R.nms_rows(bx, sc, lb, meta, 0.5, 10, 10000, False)["keep"].tolist()
    agn = R.nms_rows(bx, sc, lb, meta, 0.5, 10, 10000, True)["keep"].tolist()
    per_label = R.nms_rows(bx, sc, lb, meta, 0.5, 10, 2, True)["keep"].tolist()      # 4 >= split_thr: per label, boxes as they are
    assert aware == [0, 1, 2] and agn == [0, 2] and per_label == [0, 1, 2]
    r = R.nms_rows(bx, sc, lb, [1, 2, 0, 2, 4, 4, 100, 0], 0.5, 10, 10000, True)      # Uni order: rescale after NMS, then clamp
    assert r["bboxes"].tolist() == [[0, 0, 4, 2], [4, 12, 4, 14.5]]


def test_refusals_stay_and_the_keywords_are_stored():
    from wedetect_amd.detector import YOLOWorldDetector
    with pytest.raises(NotImplementedError, match="class_agnostic"):
        YOLOWorldDetector("nano", test_cfg=dict(nms=dict(type="nms", iou_threshold=0.5, class_agnostic=True)))
    with pytest.raises(NotImplementedError, match="multi_label"):
        YOLOWorldDetector("nano", test_cfg=dict(multi_label=False))
    with pytest.raises(NotImplementedError, match="best_class"):
        YOLOWorldDetector("nano", agnostic_nms=True)
    d = YOLOWorldDetector("nano")
    assert d.best_class is False and d.agnostic_nms is False and d._best_kw() == {}
    d = YOLOWorldDetector("nano", best_class=True, agnostic_nms=True)
    assert d.best_class is True and d.agnostic_nms is True and d._best_kw() == dict(best_class=True, agnostic_nms=True)
    assert d.test_cfg == dict(multi_label=True, nms_pre=30000, score_thr=0.001, nms=dict(type="nms", iou_threshold=0.7), max_per_img=300)
    for fn, what in ((lambda: d.predict_tiled(np.zeros((64, 64, 3), np.uint8)), "predict_tiled"), (lambda: d.predict_views([], {}), "predict_views")):
        with pytest.raises(NotImplementedError, match="best_class"):
            fn()


def test_keywords_reach_the_detector_from_a_config_and_from_the_scripts():
    import json

    from wedetect_amd.config import build_detector
    ref = json.load(open(os.path.join(ROOT, "tests", "golden", "model_cfgs.json")))["base"]["model"]
    m = build_detector(dict(ref, best_class=True, agnostic_nms=True))
    assert m.best_class and m.agnostic_nms
    assert not build_detector(ref).best_class
    import infer_wedetect
    import test as test_script
    a = infer_wedetect.parse_args(["--config", "c", "--best-class", "--agnostic-nms"])
    assert a.best_class and a.agnostic_nms
    for argv in (["--config", "c", "--agnostic-nms"], ["--config", "c", "--best-class", "--tile", "640"]):
        with pytest.raises(SystemExit):
            infer_wedetect.parse_args(argv)
    a = test_script.parse_args(["cfg.py", "ckpt.pth", "--best-class"])
    assert a.best_class and not a.agnostic_nms
    for argv in (["cfg.py", "ckpt.pth", "--agnostic-nms"], ["cfg.py", "ckpt.pth", "--best-class", "--aug-test"]):
        with pytest.raises(SystemExit):
            test_script.parse_args(argv)


def test_header_entry_list_matches_the_binding_and_every_entry_has_an_extent_case():
    from tests.abi_decl import declared
    from tests.test_cpu_abi import check_header
    from wedetect_amd import best as BS
    from wedetect_amd import build as WB
    hdr = open(os.path.join(ROOT, "include", "wedetect_hip_best.h")).read()
    names = list(declared("wedetect_hip_best.h"))
    assert sorted(names) == sorted(BS.EXPORTS)
    check_header("wedetect_hip_best.h")                       # argtypes / restype against the prototypes
    assert "wedetect_hip_best.h" in WB.PUBLIC_HEADERS and "best.hip" in WB.SOURCES
    assert re.search(r"#define\s+WD_NMS_MMCV_AGNOSTIC\s+3\b", hdr) and BS.NMS_MMCV_AGNOSTIC == 3
    assert BS.LIB.wd_best_abi_version() == BS.BEST_ABI_VERSION == 1
    from wedetect_amd import lib as L
    assert L.LIB.wd_abi_version() == L.ABI_VERSION == 15       # the main ABI stays
    ext = open(os.path.join(ROOT, "tests", "test_gpu_best_extents.py")).read()
    for n in names:
        assert n == "wd_best_abi_version" or f'"{n}"' in ext, f"{n}: no guard-band case"


def test_wrappers_are_declared_to_the_happens_before_checker():
    from tests import hazards as H
    assert {"best.best_similarity_split", "best.best_rows", "best.best_unpack", "best.nms_gather_labeled"} <= set(H.ACCESS)
    cite = [c for w, _, c in H.BENIGN if w == "best.best_similarity_split"]
    assert len(cite) == 1
    ln = int(re.search(r"split_gemm_p8\.hip:(\d+)", cite[0]).group(1))
    src = open(os.path.join(ROOT, "wedetect_amd", "csrc", "split_gemm_p8.hip")).read().splitlines()
    assert "*p.range_flag = 1u;" in src[ln - 1]


def test_mmcv_agnostic_restatement_matches_the_oracle_on_random_boxes():
    g = np.random.default_rng(12)
    n = 200
    ctr, wh = g.random((n, 2), dtype=np.float32) * 100, g.random((n, 2), dtype=np.float32) * 40 + 2
    bx = np.concatenate([ctr - wh / 2, ctr + wh / 2], 1).astype(np.float32)
    sc = np.sort(g.random(n, dtype=np.float32))[::-1].copy()
    lb = g.integers(0, 5, n)
    meta = [0, 0, 0, 1, 1, 1e9, 1e9, 1]
    for split_thr in (64, 10000):
        for agn in (False, True):
            k = R.nms_rows(bx, sc, lb, meta, 0.5, 300, split_thr, agn)["keep"]
            want = opp.mmcv_batched_nms(bx, sc, lb, dict(type="nms", iou_threshold=0.5, split_thr=split_thr, class_agnostic=agn), max_keep=300)
            assert np.array_equal(k, want)
