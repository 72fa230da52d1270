"""The n best names of a region on the CPU: the numpy restatement (tests/topn_ref.py) against brute force and against the
best-class restatement, the key and its tie rule, a step-by-step model of the merge the kernels run under random interleavings,
the public switches and refusals, the header against the binding."""
import os
import re

import numpy as np
import pytest

import tests.best_hazards  # noqa: F401
import tests.topn_hazards  # noqa: F401  (declares the wrappers of wedetect_amd/topn.py to tests/hazards.py)
from tests import best_ref as BR
from tests import topn_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _tied_rows(rows=200, k=37, seed=4):
    g = np.random.default_rng(seed)
    sc = (np.round(g.random((rows, k), dtype=np.float32) * 16) / 16).astype(np.float32)      # 17 levels over 37 classes: ties in every row
    sc[3] = 0.5                                              # a constant row: classes 0, 1, 2, ...
    sc[4, [30, 2, 17]] = 2.0                                 # three classes tie at the top: 2, 17, 30
    return sc


def test_top_n_equals_brute_force_and_the_best_class_for_n_1():
    sc = _tied_rows()
    for n in (1, 3, 8):
        s, lab = R.top_n(sc, n)
        s2, lab2 = R.top_n_loop(sc, n)
        assert np.array_equal(s.view(np.uint32), s2.view(np.uint32)) and np.array_equal(lab, lab2)
        assert bool((np.diff(s, axis=1) <= 0).all())
    s, lab = R.top_n(sc, 8)
    assert lab[3].tolist() == list(range(8)) and lab[4, :3].tolist() == [2, 17, 30]
    assert int(((np.diff(s, axis=1) == 0) & (np.diff(lab, axis=1) > 0)).sum()) > 100      # equal scores: class ascending, seen often
    assert not bool(((np.diff(s, axis=1) == 0) & (np.diff(lab, axis=1) <= 0)).any())
    best, arg = BR.best_class(sc)
    s1, l1 = R.top_n(sc, 1)
    assert np.array_equal(s1[:, 0], best) and np.array_equal(l1[:, 0], arg)
    # fewer classes than slots: the rest is empty
    s, lab = R.top_n(sc[:, :3], 5)
    assert bool((lab[:, 3:] == -1).all()) and bool((s[:, 3:] == 0).all()) and bool((lab[:, :3] >= 0).all())


def test_key_round_trip_and_tie_rule():
    from wedetect_amd import best as BS
    from wedetect_amd import topn as TN
    sc = _tied_rows()
    s, lab = R.top_n(sc[:, :5], 8)                           # three empty slots per row
    key = TN.pack(s, lab + np.where(lab >= 0, 1000, 0))
    assert key.dtype == np.uint64 and key.shape == (200, 8)
    assert bool((key[:, 5:] == 0).all()) and bool((key[:, :5] != 0).all())
    s2, lab2 = TN.unpack(key)
    assert np.array_equal(s2.view(np.uint32), s.view(np.uint32)) and np.array_equal(lab2[:, :5], lab[:, :5] + 1000) and bool((lab2[:, 5:] == -1).all())
    # slot 0 is the best-class key, bit for bit
    best, arg = BR.best_class(sc[:, :5])
    assert np.array_equal(key[:, 0], BS.pack_key(best.view(np.uint32), arg + 1000))
    # the list is the row's keys in descending unsigned order: score first, then the LOWER class
    allk = BS.pack_key(sc.view(np.uint32), np.arange(sc.shape[1])[None, :])
    want = -np.sort(-allk.astype(np.int64), axis=1)[:, :8]   # keys of scores in [0, 2] are below 2^63
    s8, l8 = R.top_n(sc, 8)
    assert np.array_equal(TN.pack(s8, l8).astype(np.int64), want)
    # merging disjoint chunks in any order = the n largest of the union
    parts = [TN.pack(*[a + (0 if i == 0 else np.where(a >= 0, lo, 0)) for i, a in enumerate(R.top_n(sc[:, lo:hi], 8))])
             for lo, hi in ((20, 37), (0, 9), (9, 20))]
    merged = -np.sort(-np.concatenate(parts, axis=1).astype(np.int64), axis=1)[:, :8]
    assert np.array_equal(merged, want)


@pytest.mark.parametrize("n", [1, 3, 8])
def test_merge_model_ends_in_the_sorted_top_n_under_every_interleaving(n):
    """64 distinct keys, up to 8 producers with disjoint shares, 1 000 random interleavings of their atomic steps; producers that
    prune on a bound read long before they offer, and re-read it between offers, included."""
    g = np.random.default_rng(100 + n)
    stale_seen = 0
    for trial in range(1000):
        keys = (g.permutation(5000)[:64] + 1).tolist()       # distinct, non-zero
        n_prod = int(g.integers(1, 9))
        owner = g.integers(0, n_prod, 64)
        slots = [0] * n
        prods = []
        for p in range(n_prod):
            stale = bool(g.integers(0, 2))
            stale_seen += stale
            prods.append(R.inserter(slots, [k for k, o in zip(keys, owner) if o == p], n, stale))
        if trial % 3 == 0:                                   # a second wave of producers that start when the slots are full: their bound prunes
            R.run_interleaved(prods, g)
            late = (g.permutation(5000)[:16] + 5001).tolist() + (g.permutation(2000)[:16] + 10001).tolist()
            keys = keys + late
            prods = [R.inserter(slots, late[i::4], n, True) for i in range(4)]
        R.run_interleaved(prods, g)
        assert slots == sorted(keys, reverse=True)[:n], (trial, slots)
    assert stale_seen > 1000


def test_merge_is_not_idempotent_a_key_offered_twice_takes_two_slots():
    """The contract of the header: the chunks of a step are DISJOINT.  (A maximum would not care.)"""
    g = np.random.default_rng(7)
    slots = [0] * 3
    R.run_interleaved([R.inserter(slots, [50, 40, 30], 3, False), R.inserter(slots, [50, 20], 3, False)], g)
    assert slots == [50, 50, 40]


def test_public_switches_and_refusals():
    from wedetect_amd.detector import YOLOWorldDetector
    from wedetect_amd import topn as TN
    with pytest.raises(ValueError, match="best_class"):
        YOLOWorldDetector("nano", top_names=3)
    for bad in (-1, 9, 2.0, True):
        with pytest.raises(ValueError, match="0..8"):
            YOLOWorldDetector("nano", best_class=True, top_names=bad)
    d = YOLOWorldDetector("nano", best_class=True)
    assert d.top_names == 0 and d._best_kw() == dict(best_class=True, agnostic_nms=False)
    d = YOLOWorldDetector("nano", best_class=True, top_names=5)
    assert d.top_names == 5 and d._best_kw() == dict(best_class=True, agnostic_nms=False)
    for fn, what in ((lambda: d.predict_stream([], 1, []), "predict_stream"), (lambda: d.predict_tiled(np.zeros((64, 64, 3), np.uint8)), "predict_tiled"),
                     (lambda: d.predict_views([], {}), "predict_views")):
        with pytest.raises(NotImplementedError, match="top_names"):
            fn()
    for bad in (0, 9, "3"):
        with pytest.raises(ValueError):
            TN.check_n_top(bad)
    assert TN.check_n_top(8) == 8 and TN.check_n_top(0, lo=0) == 0


def test_tower_detect_refuses_top_names_before_any_device_work():
    """ImageTower.detect validates the keyword first: the checks need neither a tower nor a device."""
    from wedetect_amd.engine import ImageTower
    kw = dict(normalize_text=True, score_thr=0.1)
    with pytest.raises(ValueError, match="best_class"):
        ImageTower.detect(None, None, None, None, top_names=3, **kw)
    for bad in (-1, 9, 1.5):
        with pytest.raises(ValueError, match="0..8"):
            ImageTower.detect(None, None, None, None, best_class=True, top_names=bad, **kw)


def test_keyword_reaches_the_detector_from_a_config_and_from_the_script():
    import json

    import infer_wedetect
    from wedetect_amd.config import build_detector
    ref = json.load(open(os.path.join(ROOT, "tests", "golden", "model_cfgs.json")))["base"]["model"]
    m = build_detector(dict(ref, best_class=True, top_names=4))
    assert m.best_class and m.top_names == 4
    assert build_detector(ref).top_names == 0
    a = infer_wedetect.parse_args(["--config", "c", "--best-class", "--top-names", "5"])
    assert a.best_class and a.top_names == 5
    assert infer_wedetect.parse_args(["--config", "c", "--best-class"]).top_names == 0
    for argv in (["--config", "c", "--top-names", "3"], ["--config", "c", "--best-class", "--top-names", "9"]):
        with pytest.raises(SystemExit) as ei:
            infer_wedetect.parse_args(argv)
        assert ei.value.code == 2


def test_script_says_why_it_refuses_top_names_without_best_class(capsys):
    import infer_wedetect
    with pytest.raises(SystemExit):
        infer_wedetect.parse_args(["--config", "c", "--top-names", "3"])
    assert "--top-names needs --best-class" in capsys.readouterr().err


def test_header_prototypes_match_the_binding_and_every_entry_has_an_extent_case():
    from tests.abi_decl import declared
    from tests.test_cpu_abi import check_header
    from wedetect_amd import build as WB
    from wedetect_amd import lib as L
    from wedetect_amd import topn as TN
    hdr = open(os.path.join(ROOT, "include", "wedetect_hip_topn.h")).read()
    protos = declared("wedetect_hip_topn.h")
    assert sorted(protos) == sorted(TN.EXPORTS) and all(ret == "int" for ret, _ in protos.values())
    assert "wedetect_hip_topn.h" in WB.PUBLIC_HEADERS and "topn.hip" in WB.SOURCES
    check_header("wedetect_hip_topn.h")                       # argtypes / restype against the prototypes
    assert re.search(r"#define\s+WD_TOPN_MAX\s+8\b", hdr) and TN.TOPN_MAX == 8
    assert TN.LIB.wd_topn_abi_version() == TN.TOPN_ABI_VERSION == 1
    assert L.LIB.wd_abi_version() == L.ABI_VERSION == 15       # the main ABI stays
    for name in protos:                                       # each entry states its extents ...
        if name != "wd_topn_abi_version":
            doc = hdr[: hdr.index(f"int {name}(")].rsplit("/* ----", 1)[1]
            assert "Extents:" in doc, name
    ext = open(os.path.join(ROOT, "tests", "test_gpu_topn_extents.py")).read()
    for name in protos:                                       # ... and has a guard-band case
        assert name == "wd_topn_abi_version" or f'"{name}"' in ext, f"{name}: no guard-band case"


def test_wrappers_are_declared_to_the_happens_before_checker():
    from tests import hazards as H
    assert {"topn.topn_similarity_split", "topn.topn_rows", "topn.topn_unpack", "topn.topn_kept"} <= set(H.ACCESS)
    cite = [c for w, _, c in H.BENIGN if w == "topn.topn_similarity_split"]
    assert len(cite) == 1
    ln = int(re.search(r"split_gemm_p8\.hip:(\d+)", cite[0]).group(1))
    src = open(os.path.join(ROOT, "wedetect_amd", "csrc", "split_gemm_p8.hip")).read().splitlines()
    assert "*p.range_flag = 1u;" in src[ln - 1]
    body = max(i for i, l in enumerate(src) if "p8_topn_epilogue(" in l and l.startswith("__device__"))
    assert body < ln - 1 and not any(l.startswith("__device__") and "epilogue(" in l for l in src[body + 1: ln])     # inside the top-n epilogue
