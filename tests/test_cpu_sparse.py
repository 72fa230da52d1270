"""Sparse scores on the CPU: the numpy restatement (tests/sparse_ref.py) against the oracle's filter_scores_and_topk on the
fixture the reference wrote (tests/golden/filter_topk.npz), the 64-bit key's order, the select rules, the header against the
binding, the public switches and their refusals."""
import os
import re

import numpy as np
import pytest

import tests.sparse_hazards  # noqa: F401  (declares the wrappers of wedetect_amd/sparse.py to tests/hazards.py)
from oracle import postprocess as opp
from tests import sparse_ref as R
from tests.util import golden

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_sparse_ref_reproduces_the_reference_fixture_position_by_position():
    fx = golden("filter_topk.npz")
    for name in ("ties", "trunc", "empty", "all_equal"):
        sc, thr, topk = fx[f"{name}.in"], float(fx[f"{name}.thr"]), int(fx[f"{name}.topk"])
        s, lab, anc = R.filter_topk(sc, thr, topk)
        os_, ol, oa = opp.filter_scores_and_topk(sc, thr, topk)
        for got, want, ref in ((s, os_, fx[f"{name}.scores"]), (lab, ol, fx[f"{name}.labels"]), (anc, oa, fx[f"{name}.anchors"])):
            assert np.array_equal(got, want) and np.array_equal(got, ref)
        assert s.dtype == np.float32
    assert fx["empty.scores"].shape[0] == 0
    assert int((np.diff(fx["ties.scores"]) == 0).sum()) > 0      # equal scores inside the fixture's list
    n_valid = int((fx["trunc.in"] > np.float32(fx["trunc.thr"])).sum())
    assert n_valid > int(fx["trunc.topk"]) == fx["trunc.scores"].shape[0]          # the cut lies inside the list


def test_key_order_is_score_descending_then_flat_ascending():
    g = np.random.default_rng(5)
    s = (np.round(g.random(4096, dtype=np.float32) * 64) / 64).astype(np.float32)      # many equal scores
    s[:4] = (0.0, 1.0, np.float32(1e-45), 0.5)                   # +0, the largest score, a denormal
    flat = g.permutation(2 ** 31 - 2 - np.arange(4096))          # unique, up to 2^31 - 1
    flat[:2] = (0, 2 ** 31 - 1)
    key = R.pack_key(s, flat)
    assert key.dtype == np.uint64 and np.array_equal(key, ((~s.view(np.uint32)).astype(np.uint64) << np.uint64(32)) | flat.astype(np.uint64))
    s2, f2 = R.unpack_key(key)
    assert np.array_equal(s2.view(np.uint32), s.view(np.uint32)) and np.array_equal(f2, flat)
    order = np.lexsort((flat, -s.astype(np.float64)))            # score desc, then flat asc
    assert np.array_equal(np.argsort(key, kind="stable"), order)
    assert int((np.diff(s[order]) == 0).sum()) > 1000


def test_lists_and_select_rules():
    g = np.random.default_rng(6)
    sc = (np.round(g.random((2 * 50, 9), dtype=np.float32) * 16) / 16).astype(np.float32)
    keys, seen = R.lists(sc, 2, 0.5)
    for b in range(2):
        s, lab, anc = opp.filter_scores_and_topk(sc[b * 50:(b + 1) * 50], 0.5, 10 ** 6)
        assert seen[b] == s.shape[0] and np.array_equal(keys[b], R.pack_key(s, anc * 9 + lab))
        # cut into class chunks, in any order: the same set
        parts = [R.image_list(sc[b * 50:(b + 1) * 50, a:z], 0.5, n_cls_total=9, cls_offset=a) for a, z in ((5, 9), (0, 2), (2, 5))]
        assert np.array_equal(np.sort(np.concatenate(parts)), keys[b])
    k0 = keys[0][::-1].copy()                                    # any order in
    idx, s, n, status = R.select(k0, seen[0], False, 1024, 100)
    want = opp.filter_scores_and_topk(sc[:50], 0.5, 100)
    assert status == 0 and n == 100 and idx.shape == (128,) and np.array_equal(s[:n], want[0])
    assert np.array_equal(idx[:n], want[2] * 9 + want[1]) and bool((idx[n:] == -1).all()) and not s[n:].any()
    assert R.select(k0[:64], seen[0], False, 64, 100)[2:] == (0, 1) and seen[0] > 64          # overflow: nothing is used
    assert R.select(k0, seen[0], True, 1024, 100)[2:] == (-1, 2)                                 # non-finite wins
    assert R.select(k0[:0], 0, False, 1024, 100)[2:] == (0, 0)


def test_header_entry_list_matches_the_binding_and_every_entry_has_an_extent_case():
    from tests.abi_decl import declared
    from tests.test_cpu_abi import check_header
    from wedetect_amd import build as WB
    from wedetect_amd import lib as L
    from wedetect_amd import sparse as SP
    hdr = open(os.path.join(ROOT, "include", "wedetect_hip_sparse.h")).read()
    names = list(declared("wedetect_hip_sparse.h"))
    assert sorted(names) == sorted(SP.EXPORTS)
    check_header("wedetect_hip_sparse.h")                        # argtypes / restype against the prototypes
    assert "wedetect_hip_sparse.h" in WB.PUBLIC_HEADERS and "sparse.hip" in WB.SOURCES
    assert "sparse.hip" in WB.NO_SCRATCH and "sparse.hip" in WB.ASM_VMEM_SOURCES and "split_gemm_p8_kernel" in WB.NO_SCRATCH["split_gemm_p8.hip"]
    for name, val in (("WD_SPARSE_OK", 0), ("WD_SPARSE_OVERFLOW", 1), ("WD_SPARSE_NONFINITE", 2)):
        assert re.search(rf"#define\s+{name}\s+{val}\b", hdr)
    assert (SP.STATUS_OK, SP.STATUS_OVERFLOW, SP.STATUS_NONFINITE) == (R.STATUS_OK, R.STATUS_OVERFLOW, R.STATUS_NONFINITE) == (0, 1, 2)
    assert SP.LIB.wd_sparse_abi_version() == SP.SPARSE_ABI_VERSION == 1
    assert L.LIB.wd_abi_version() == L.ABI_VERSION == 15         # the main ABI stays
    from wedetect_amd import best as BS
    assert BS.LIB.wd_best_abi_version() == 1
    for n in names:                                              # every entry documents its extents and has a guard-band case
        assert n == "wd_sparse_abi_version" or len(re.findall(rf"\* {n} —.*?Extents:", hdr, flags=re.S)) == 1, n
    ext = open(os.path.join(ROOT, "tests", "test_gpu_sparse_extents.py")).read()
    for n in names:
        assert n == "wd_sparse_abi_version" or f'"{n}"' in ext, f"{n}: no guard-band case"
    assert SP.list_capacity(65536, 30000) == 65536 and SP.list_capacity(1024, 30000) == 32768 and SP.list_capacity(1000, 1000) == 1024
    with pytest.raises(ValueError):
        SP.list_capacity((1 << 20) + 1, 1000)


def test_wrappers_are_declared_to_the_happens_before_checker():
    from tests import hazards as H
    assert {"sparse.sparse_similarity_split", "sparse.sparse_rows", "sparse.sparse_select"} <= set(H.ACCESS)
    cite = [c for w, _, c in H.BENIGN if w == "sparse.sparse_similarity_split"]
    assert len(cite) == 1
    ln = int(re.search(r"split_gemm_p8\.hip:(\d+)", cite[0]).group(1))
    src = open(os.path.join(ROOT, "wedetect_amd", "csrc", "split_gemm_p8.hip")).read().splitlines()
    assert "*p.range_flag = 1u;" in src[ln - 1]
    body = "\n".join(src[ln - 60: ln])
    assert "p8_sparse_epilogue(" in body


def test_refusals_and_the_keywords_are_stored():
    from wedetect_amd.detector import YOLOWorldDetector
    with pytest.raises(ValueError, match="best_class"):
        YOLOWorldDetector("nano", best_class=True, sparse_scores=True)
    with pytest.raises(ValueError, match="sparse_cap"):
        YOLOWorldDetector("nano", sparse_scores=True, sparse_cap=(1 << 20) + 1)
    d = YOLOWorldDetector("nano")
    assert d.sparse_scores is False and d.sparse_cap == 65536 and d._sparse_kw() == {} and d._best_kw() == {}
    d = YOLOWorldDetector("nano", sparse_scores=True, sparse_cap=4096)
    assert d.sparse_scores is True and d._sparse_kw() == dict(sparse_scores=True, sparse_cap=4096) and d._best_kw() == {}
    assert d.test_cfg == dict(multi_label=True, nms_pre=30000, score_thr=0.001, nms=dict(type="nms", iou_threshold=0.7), max_per_img=300)
    calls = ((lambda: d.predict_tiled(np.zeros((64, 64, 3), np.uint8)), "predict_tiled"), (lambda: d.predict_views([], {}), "predict_views"),
             (lambda: d.predict_stream([], 1, []), "predict_stream"))
    for fn, what in calls:
        with pytest.raises(NotImplementedError, match=rf"{what} with sparse_scores=True"):
            fn()


def test_keywords_reach_the_detector_from_a_config_and_from_the_scripts():
    import json

    from wedetect_amd.config import build_detector
    ref = json.load(open(os.path.join(ROOT, "tests", "golden", "model_cfgs.json")))["base"]["model"]
    m = build_detector(dict(ref, sparse_scores=True, sparse_cap=2048))
    assert m.sparse_scores and m.sparse_cap == 2048 and not m.best_class
    assert not build_detector(ref).sparse_scores
    with pytest.raises(ValueError):
        build_detector(dict(ref, sparse_scores=True, best_class=True))
    import infer_wedetect
    import test as test_script
    a = infer_wedetect.parse_args(["--config", "c", "--sparse-scores"])
    assert a.sparse_scores and a.sparse_cap == 65536 and not a.best_class
    assert infer_wedetect.parse_args(["--config", "c", "--sparse-scores", "--sparse-cap", "1024"]).sparse_cap == 1024
    assert not infer_wedetect.parse_args(["--config", "c"]).sparse_scores
    for argv in (["--config", "c", "--sparse-scores", "--best-class"], ["--config", "c", "--sparse-scores", "--tile", "640"]):
        with pytest.raises(SystemExit):
            infer_wedetect.parse_args(argv)
    a = test_script.parse_args(["cfg.py", "ckpt.pth", "--sparse-scores", "--sparse-cap", "4096"])
    assert a.sparse_scores and a.sparse_cap == 4096
    for extra in (["--best-class"], ["--aug-test"], ["--loader", "stream"]):
        with pytest.raises(SystemExit):
            test_script.parse_args(["cfg.py", "ckpt.pth", "--sparse-scores", *extra])
