"""Exemplar prompts on the CPU: the numpy restatement (tests/exemplar_ref.py) against a brute-force loop and hand-made vectors, the
header against the binding and the build lists, the argument refusals, the detector's and the script's host side."""
import ctypes
import hashlib
import os
import re

import numpy as np
import pytest

import tests.exemplar_hazards  # noqa: F401  (declares the wrappers of wedetect_amd/exemplar.py to tests/hazards.py)
from tests import exemplar_ref as R
from tests.abi_decl import declared

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "wedetect_hip_exemplar.h")
f32 = np.float32
IDENT = np.array([[0, 0, 0, 1, 1, 64, 64, 0]], f32)


# ------------------------------------------------------------------------------------------------------------ reference
def test_assign_equals_the_brute_force_loop_on_random_boxes():
    g = np.random.default_rng(11)
    B, N, max_ex = 3, 300, 5
    xy = g.random((B, N, 2), dtype=f32) * 56
    wh = np.round(g.random((B, N, 2), dtype=f32) * 6 + 2)                    # few distinct sizes: IoU ties occur
    boxes = np.concatenate([np.round(xy), np.round(xy) + wh], axis=2).astype(f32)
    boxes[1, 100:110] = boxes[1, 5]                                          # duplicates at distant anchors
    ex = np.concatenate([np.round(xy[:, :max_ex] * 2), np.round(xy[:, :max_ex] * 2) + 2 * wh[:, :max_ex]], axis=2).astype(f32)
    meta = np.array([[1.5, 2.5, 0, 0.5, 0.5, 128, 128, 0]] * B, f32)
    cnt = np.array([5, 0, 3], np.int32)
    ties = 0
    for m in (1, 4, 8):
        for thr in (0.0, 0.3):
            a, i, c = R.assign(boxes, ex, cnt, meta, m, thr)
            a2, i2, c2 = R.assign_loop(boxes, ex, cnt, meta, m, thr)
            assert np.array_equal(a, a2) and np.array_equal(i.view(np.uint32), i2.view(np.uint32)) and np.array_equal(c, c2)
            assert c.tolist() == [5 * m, 0, 3 * m] and bool((a[1] == -1).all()) and not i[1].any()
            rows = a.reshape(B, max_ex, m)
            iou = i.reshape(B, max_ex, m)
            assert bool((np.diff(iou, axis=2) <= 0).all())
            ties += int(((np.diff(iou, axis=2) == 0) & (rows[:, :, 1:] >= 0)).sum())
            assert not bool(((np.diff(iou, axis=2) == 0) & (rows[:, :, 1:] >= 0) & (np.diff(rows, axis=2) <= 0)).any())
    assert ties > 5                                                           # equal IoUs: anchor ascending, seen


def test_hand_made_vectors():
    boxes = np.array([[[0, 0, 10, 10], [100, 100, 110, 110], [0, 0, 10, 10], [0, 0, 10, 20], [np.nan, 0, 10, 10], [0, 0, 20, 20]]], f32)
    ex = np.array([[[0, 0, 10, 10], [200, 200, 210, 210], [0, 0, 20, 20]]], f32)
    # a tie in IoU: anchors 0 and 2 both have IoU 1, the lower anchor comes first; then 0.5 (anchor 3), then 0.25 (anchor 5)
    a, i, c = R.assign(boxes, ex, [3], IDENT, 4, 0.1)
    assert a[0, :4].tolist() == [0, 2, 3, 5] and i[0, :4].tolist() == [1.0, 1.0, 0.5, 0.25] and c.tolist() == [12]
    # fewer than m candidates: an example that matches nothing, and one with IoUs 1, 0.5, 0.25, 0.25
    assert a[0, 4:8].tolist() == [-1] * 4 and not i[0, 4:8].any()
    assert a[0, 8:].tolist() == [5, 3, 0, 2] and i[0, 8:].tolist() == [1.0, 0.5, 0.25, 0.25]
    # min_iou boundary: equality is not a candidate
    a, i, _ = R.assign(boxes, ex, [1], IDENT, 4, 0.5)
    assert a[0, :4].tolist() == [0, 2, -1, -1] and i[0, :4].tolist() == [1.0, 1.0, 0.0, 0.0]
    a, _, _ = R.assign(boxes, ex, [1], IDENT, 4, float(np.nextafter(f32(0.5), f32(0))))
    assert a[0, :4].tolist() == [0, 2, 3, -1]
    # the NaN box is never a candidate, whatever the threshold; ex_count = 0 and slots past ex_count are empty
    a, i, c = R.assign(boxes, ex, [0], IDENT, 2, 0.0)
    assert bool((a == -1).all()) and not i.any() and c.tolist() == [0]
    a, _, c = R.assign(boxes, ex, [1], IDENT, 8, 0.0)
    assert 4 not in a[0].tolist() and a[0, :4].tolist() == [0, 2, 3, 5] and a[0, 4:].tolist() == [-1] * 20 and c.tolist() == [8]
    # to network pixels: multiply, then add, each rounded
    mt = np.array([3.25, 1.75, 0, f32(1 / 3), f32(0.7), 0, 0, 0], f32)
    got = R.to_network([10.1, 20.2, 30.3, 40.4], mt)
    want = [f32(f32(f32(v) * s) + p) for v, s, p in zip((10.1, 20.2, 30.3, 40.4), (mt[3], mt[4], mt[3], mt[4]), (mt[0], mt[1], mt[0], mt[1]))]
    assert got.dtype == f32 and got.tolist() == [float(v) for v in want]
    # key form
    assert int(R.pack_key(f32(1.0), 7)) == (0x3F800000 << 32) | (0xFFFFFFFF - 7)


def test_pool_slot_order_support_and_empty_classes():
    g = np.random.default_rng(5)
    n_slot, dim = 6, 8
    emb = g.standard_normal((3, n_slot, dim)).astype(f32)
    anchors = np.array([3, 70, 81, -1, 65, 2], np.int32)                      # levels 0, 1, 2, -, 1, 0 with offsets 64 / 80
    iou = np.array([0.9, 0.5, 0.25, 0.0, 0.75, 0.6], f32)
    off, slot = [0, 3, 3, 5, 6], [0, 1, 2, 3, 4, 3]
    bank, sup = R.pool(emb, 64, 80, anchors, iou, off, slot)
    assert sup.tolist() == [3, 0, 1, 0] and not bank[1].any() and not bank[3].any()
    rows = [emb[0, 0], emb[1, 1], emb[2, 2]]
    acc = sum(w * (r.astype(np.float64) / np.linalg.norm(r.astype(np.float64))) for w, r in zip((0.9, 0.5, 0.25), rows))
    assert np.allclose(bank[0], acc / np.linalg.norm(acc), atol=1e-7) and abs(np.linalg.norm(bank[0]) - 1) < 1e-12
    assert np.allclose(bank[2], emb[1, 4] / np.linalg.norm(emb[1, 4].astype(np.float64)), atol=1e-7)
    # slot order within a class is the caller's list order: the same set listed otherwise sums in another order (same value here
    # up to rounding, the same support)
    bank2, sup2 = R.pool(emb, 64, 80, anchors, iou, [0, 3], [2, 0, 1])
    assert sup2.tolist() == [3] and np.allclose(bank2[0], bank[0], atol=1e-12)
    assert R.level_of([0, 63, 64, 79, 80, 83], 64, 80).tolist() == [0, 0, 1, 1, 2, 2]
    assert R.pool_bound(3) == 11 * 2.0 ** -23


# ------------------------------------------------------------------------------------------------- header, library, build
def test_library_exports_the_header_and_the_frozen_abi_is_untouched():
    from tests.test_cpu_abi import check_header
    from tests.test_cpu_tile import MAIN_HEADER_SHA256
    from wedetect_amd import build as WB
    from wedetect_amd import exemplar as EX
    from wedetect_amd import lib as L
    decl = declared("wedetect_hip_exemplar.h")
    assert sorted(decl) == sorted(EX.EXPORTS) == ["wd_exemplar_abi_version", "wd_exemplar_assign", "wd_exemplar_pool"]
    for name in decl:
        assert hasattr(L.LIB, name)
    assert EX.LIB.wd_exemplar_abi_version() == EX.EXEMPLAR_ABI_VERSION == 1
    assert L.LIB.wd_abi_version() == L.ABI_VERSION == 15
    assert hashlib.sha256(open(os.path.join(ROOT, "include", "wedetect_hip.h"), "rb").read()).hexdigest() == MAIN_HEADER_SHA256
    hdr = open(HEADER).read()
    assert re.search(r"#define\s+WD_EXEMPLAR_MAX_M\s+8\b", hdr) and EX.MAX_M == 8
    assert re.search(r"#define\s+WD_EXEMPLAR_MAX_EX\s+64\b", hdr) and EX.MAX_EX == 64
    check_header("wedetect_hip_exemplar.h")                                   # argtypes / restype against the prototypes
    for name in decl:
        if name == "wd_exemplar_abi_version":
            continue
        doc = hdr[: hdr.index(f"int {name}(")].rsplit("/* ----", 1)[1]
        assert "Extents:" in doc and "WD_ERR_BAD_ARG:" in doc, name


def test_build_lists_are_as_registered():
    from wedetect_amd import build as WB
    assert "exemplar.hip" in WB.SOURCES and "wedetect_hip_exemplar.h" in WB.PUBLIC_HEADERS
    assert WB.NO_SCRATCH["exemplar.hip"] == ["exemplar_assign_kernel", "exemplar_pool_kernel"]
    assert WB.ASM_VMEM_SOURCES["exemplar.hip"] == []
    src = open(os.path.join(WB.CSRC, "exemplar.hip")).read()
    for k in WB.NO_SCRATCH["exemplar.hip"]:
        assert re.search(r"__global__[^;{]*\b" + k + r"\(", src), k
    assert "atomic" not in src.replace("no atomics", "")                      # the selection uses no atomics


def test_argument_refusals_before_any_launch():
    from wedetect_amd import exemplar as EX
    one, odd = ctypes.c_void_p(256), ctypes.c_void_p(260)                     # non-null, never dereferenced: refused first
    nan, inf = float("nan"), float("inf")

    def assign(boxes=one, n_anchor=84, ex_boxes=one, ex_count=one, meta=one, max_ex=4, batch=2, m=4, min_iou=0.1, sel_a=one,
               sel_i=one, sel_c=one):
        return EX.LIB.wd_exemplar_assign(boxes, n_anchor, ex_boxes, ex_count, meta, max_ex, batch, m, min_iou, sel_a, sel_i, sel_c, None)

    for kw in (dict(boxes=None), dict(ex_boxes=None), dict(ex_count=None), dict(meta=None), dict(sel_a=None), dict(sel_i=None),
               dict(sel_c=None), dict(n_anchor=0), dict(batch=0), dict(batch=-1), dict(max_ex=0), dict(max_ex=65), dict(m=0), dict(m=9),
               dict(min_iou=-0.5), dict(min_iou=nan), dict(min_iou=inf), dict(boxes=odd), dict(ex_boxes=ctypes.c_void_p(258)),
               dict(batch=65536), dict(batch=40000, n_anchor=60000)):
        assert assign(**kw) == -1, kw

    def pool(level_embed=one, dim=768, off1=64, off2=80, sel_a=one, sel_i=one, n_slot=32, cls_off=one, cls_slot=one, n_cls=3,
             bank=one, support=one):
        return EX.LIB.wd_exemplar_pool(level_embed, dim, off1, off2, sel_a, sel_i, n_slot, cls_off, cls_slot, n_cls, bank, support, None)

    for kw in (dict(level_embed=None), dict(sel_a=None), dict(sel_i=None), dict(cls_off=None), dict(bank=None), dict(support=None),
               dict(n_slot=0), dict(n_cls=0), dict(dim=0), dict(dim=770), dict(dim=1028), dict(off1=0), dict(off1=80, off2=80),
               dict(level_embed=odd), dict(bank=odd), dict(support=ctypes.c_void_p(258)), dict(n_slot=1 << 20, dim=1024)):
        assert pool(**kw) == -1, kw
    for bad in (0, 9, 2.0, True, "4"):
        with pytest.raises(ValueError):
            EX.check_m(bad)
    for bad in (-0.1, nan, inf):
        with pytest.raises(ValueError):
            EX.check_min_iou(bad)
    assert EX.check_m(8) == 8 and EX.check_min_iou(0) == 0.0


def test_every_exemplar_entry_point_with_device_memory_has_an_extents_case():
    from tests.test_cpu_arena import _takes_memory
    from tests.test_gpu_exemplar_extents import CASES
    decl = declared("wedetect_hip_exemplar.h")
    covered = {c.entry for c in CASES}
    for name, params in sorted(decl.items()):
        if name == "wd_exemplar_abi_version":
            assert not _takes_memory(params) and name not in covered
            continue
        assert _takes_memory(params) and name in covered, f"{name}: exemplar entry without a case in tests/test_gpu_exemplar_extents.py"
    assert not covered - set(decl)
    ids = [c.id for c in CASES]
    assert len(ids) == len(set(ids))


def test_wrappers_are_declared_to_the_happens_before_checker():
    from tests import hazards as H
    assert {"exemplar.exemplar_assign", "exemplar.exemplar_pool"} <= set(H.ACCESS)
    assert not any(w.startswith("exemplar.") for w, _, _ in H.BENIGN)         # plain reads and writes only


# ------------------------------------------------------------------------------------------------- detector and script
def test_plan_and_detector_refusals_need_no_device():
    from wedetect_amd.detector import YOLOWorldDetector, plan_exemplars
    box = (1.0, 2.0, 30.0, 40.0)
    p = plan_exemplars([[(box, 1), ((0, 0, 5, 5), 0)], [], [((2, 2, 9, 9), 1)]], ["cup", "dog"], 2, 0.2)
    assert p["ex_boxes"].shape == (3, 2, 4) and p["ex_count"].tolist() == [2, 0, 1] and p["max_ex"] == 2 and p["m"] == 2
    # class 0: image 0 example 1; class 1: image 0 example 0, then image 2 example 0 — slot = b * (max_ex * m) + e * m + j
    assert p["cls_off"].tolist() == [0, 2, 6] and p["cls_slot"].tolist() == [2, 3, 0, 1, 8, 9]
    assert p["cls_examples"] == [[(0, 1)], [(0, 0), (2, 0)]] and p["names"] == ["cup", "dog"]
    assert plan_exemplars([[(box, 0)]])["names"] == ["exemplar_0"]
    d = YOLOWorldDetector("nano")                                             # never moved to a device: the checks come first
    for bad, what in (([[((5, 5, 5, 9), 0)]], "positive width"), ([[((5, 9, 8, 9), 0)]], "positive width"),
                      ([[((5, 5, float("nan"), 9), 0)]], "positive width"), ([[(box, 2)]], "class 0"), ([[(box, 0)], [(box, 2)]], "class 1"),
                      ([[(box, -1)]], "non-negative"), ([[]], "no example box"), ([[(box, 0)] * 65], "at most 64")):
        with pytest.raises(ValueError, match=what):
            d.exemplar_bank([None] * len(bad), None, bad)
    with pytest.raises(ValueError, match="has no example box"):
        d.exemplar_bank([None], None, [[(box, 0)]], names=["a", "b"])
    with pytest.raises(ValueError, match="outside the 1 names"):
        d.set_exemplar_bank([None], None, [[(box, 1)]], names=["a"])
    for kw in (dict(anchors_per_box=0), dict(anchors_per_box=9), dict(min_iou=-1.0)):
        with pytest.raises(ValueError):
            d.exemplar_bank([None], None, [[(box, 0)]], **kw)
    with pytest.raises(RuntimeError, match="not on a HIP device"):            # a valid request reaches the device check
        d.exemplar_bank([None], None, [[(box, 0)]])


def test_script_flags_parse_and_are_off_by_default(capsys):
    import infer_wedetect as I
    a = I.parse_args(["--config", "c"])
    assert a.exemplar_image is None and a.exemplar_boxes is None and a.exemplars is None and a.save_bank is None and a.anchors_per_box == 4
    a = I.parse_args(["--config", "c", "--text", "x", "--exemplar-image", "e.jpg", "--exemplar-boxes", "1,2,30,40:cup; 5,5,9,9:dog;2,2,8,8:cup",
                      "--anchors-per-box", "2", "--save-bank", "o.pt"])
    assert a.exemplars == (["cup", "dog"], [((1.0, 2.0, 30.0, 40.0), 0), ((5.0, 5.0, 9.0, 9.0), 1), ((2.0, 2.0, 8.0, 8.0), 0)])
    assert a.anchors_per_box == 2 and a.save_bank == "o.pt" and a.exemplar_image == "e.jpg"
    for argv, why in ((["--exemplar-boxes", "1,2,3,4:a"], "go together"), (["--exemplar-image", "e.jpg"], "go together"),
                      (["--exemplar-image", "e.jpg", "--exemplar-boxes", "1,2,3:a"], "x1,y1,x2,y2:name"),
                      (["--exemplar-image", "e.jpg", "--exemplar-boxes", "1,2,3,4"], "x1,y1,x2,y2:name"),
                      (["--exemplar-image", "e.jpg", "--exemplar-boxes", "5,2,3,4:a"], "positive width"),
                      (["--exemplar-image", "e.jpg", "--exemplar-boxes", "1,2,3,4:a", "--anchors-per-box", "9"], "1 .. 8"),
                      (["--exemplar-image", "e.jpg", "--exemplar-boxes", "1,2,3,4:a", "--prompt-groups"], "--prompt-groups"),
                      (["--save-bank", "o.pt"], "needs --exemplar-boxes")):
        with pytest.raises(SystemExit) as ei:
            I.parse_args(["--config", "c"] + argv)
        assert ei.value.code == 2 and why in capsys.readouterr().err
