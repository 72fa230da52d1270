"""Test-time augmentation without a GPU: tests/views_ref.py against its brute-force twin and on hand-made vectors, the
TestTimeAug / RandomFlip / DetTTAModel plumbing, test.py's flags and default TTA pipeline, the views header and its binding,
and the coverage rule of the extent tests applied to the new header."""
import ctypes
import fnmatch
import hashlib
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from tests import views_ref as R  # noqa: E402
from tests.abi_decl import declared  # noqa: E402

VIEWS_HEADER = "wedetect_hip_views.h"
# sha256 of include/wedetect_hip.h at ABI 15 (tests/test_cpu_feed.py and tests/test_cpu_tile.py pin the same)
MAIN_HEADER_SHA256 = "2b62a824664907f02d66fef8abe43f4c50fa0703c00814e15a08129143937784"


def _entry():
    import importlib.util
    spec = importlib.util.spec_from_file_location("wd_test_entry_views", os.path.join(ROOT, "test.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


# ------------------------------------------------------------------------------------------------------------- views_ref
def _merge(c, n_cls, iou, split_thr, max_out, **kw):
    return R.merge(c["boxes"], c["scores"], c["labels"], c["counts"], c["view_flip"], c["img_wh"], n_cls, iou, split_thr, max_out, **kw)


def _brute(c, n_cls, iou, split_thr, max_out):
    return R.merge_brute(c["boxes"], c["scores"], c["labels"], c["counts"], c["view_flip"], c["img_wh"], n_cls, iou, split_thr, max_out)


@pytest.mark.parametrize("V", range(1, 9))
def test_views_ref_merge_equals_the_brute_force_loop(V):
    """Seeded inputs, V = 1 .. 8, the agnostic and the per-class branch, and a max_out that truncates."""
    c = R.merge_inputs(V, 2, 24, seed=V, counts="mixed")
    for split_thr, max_out in ((10000, 300), (8, 300), (10000, 5)):
        out = _merge(c, 80, 0.5, split_thr, max_out)
        assert R.brute_equals(out, _brute(c, 80, 0.5, split_thr, max_out)), (V, split_thr, max_out)
        n = out["count"]
        assert int(n.max()) >= 1 and (max_out != 5 or bool((n == 5).all()))
        if split_thr == 8:
            assert bool((c["counts"].clip(0).sum(0) >= 8).all())               # every image takes the per-class branch
        for b in range(2):
            assert bool((np.diff(out["scores"][b, :n[b]]) <= 0).all())
            assert bool((out["src"][b, n[b]:] == -1).all()) and bool((out["labels"][b, n[b]:] == -1).all())
            assert not out["boxes"][b, n[b]:].any() and not out["scores"][b, n[b]:].any()
    if V > 1:
        full = _merge(c, 80, 0.5, 10000, 300)
        assert int(full["cross_view"].sum()) >= 1 and int(((full["per_view"] > 0).sum(1) >= 2).sum()) >= 1


GPU_CASES = [(1, 1, 5, "full", [0], 1, 10000, 300), (2, 1, 8, "full", [1, 0], 80, 10000, 300), (4, 2, 64, "mixed", [0, 1, 2, 3], 80, 8, 7)]


@pytest.mark.parametrize("V,B,max_in,counts,flips,n_cls,split_thr,max_out", GPU_CASES, ids=[f"{c[0]}x{c[1]}x{c[2]}" for c in GPU_CASES])
def test_small_gpu_cases_meet_their_witnesses_and_the_brute_force_loop(V, B, max_in, counts, flips, n_cls, split_thr, max_out):
    """The small cases of tests/test_gpu_views.py, on the same seeds (the large ones are checked there, by the reference
    alone, before the device is asked)."""
    c = R.merge_inputs(V, B, max_in, seed=V * 100 + B, counts=counts, flips=flips, n_cls=n_cls)
    out = _merge(c, n_cls, 0.5, split_thr, max_out)
    assert R.brute_equals(out, _brute(c, n_cls, 0.5, split_thr, max_out))
    assert bool((c["img_wh"] % 2 == 1).all())
    if V > 1:
        assert int(out["cross_view"].sum()) >= 1 and int(((out["per_view"] > 0).sum(1) >= 2).sum()) >= 1
    beyond = c["scores"][0, 0, c["counts"][0, 0]:]
    assert bool(np.isnan(beyond).all())                      # garbage beyond each count
    if max_in >= 64:
        lab = np.concatenate([c["labels"][v, b, :c["counts"][v, b]] for v in range(V) for b in range(B)])
        assert bool(((lab < 0) | (lab >= n_cls)).any())      # labels outside the range, inside the counts


def _hand(W=641.0, H=427.0):
    c = dict(boxes=np.full((2, 1, 4, 4), np.nan, np.float32), scores=np.full((2, 1, 4), np.nan, np.float32),
             labels=np.full((2, 1, 4), 2 ** 30, np.int32), counts=np.asarray([[1], [2]], np.int32),
             view_flip=np.asarray([1, 0], np.int32), img_wh=np.asarray([[W, H]], np.float32))
    c["boxes"][0, 0, 0] = (W - 110.25, 50, W - 10.5, 90)     # the flipped view sees (10.5, 50, 110.25, 90) mirrored
    c["boxes"][1, 0, :2] = [(10.5, 50, 110.25, 90), (300, 300, 340, 360)]
    c["labels"][0, 0, 0], c["labels"][1, 0, :2] = 3, (3, 3)
    return c


def test_views_ref_on_hand_made_vectors():
    # a box in the flipped view and its mirror in the plain view with a LOWER score: the flipped view's row survives
    c = _hand()
    c["scores"][0, 0, 0], c["scores"][1, 0, :2] = 0.9, (0.8, 0.5)
    out = _merge(c, 80, 0.5, 10000, 100)
    assert out["count"].tolist() == [2] and out["src"][0, :2].tolist() == [0, 5] and out["cross_view"].tolist() == [1]
    assert out["boxes"][0, 0].tolist() == [10.5, 50, 110.25, 90] and out["per_view"].tolist() == [[1, 1]]
    assert R.brute_equals(out, _brute(c, 80, 0.5, 10000, 100))
    # the other way round: the plain view's row (slot 4) survives
    c["scores"][0, 0, 0], c["scores"][1, 0, 0] = 0.7, 0.8
    out = _merge(c, 80, 0.5, 10000, 100)
    assert out["src"][0, :2].tolist() == [4, 5] and out["cross_view"].tolist() == [1]
    # an exact score tie goes to the lower slot
    c["scores"][0, 0, 0] = c["scores"][1, 0, 0] = 0.75
    out = _merge(c, 80, 0.5, 10000, 100)
    assert out["src"][0, :2].tolist() == [0, 5] and R.brute_equals(out, _brute(c, 80, 0.5, 10000, 100))
    # different labels: both stay (class-aware offsets); a label outside the range: skipped
    c["labels"][1, 0, 0] = 4
    assert _merge(c, 80, 0.5, 10000, 100)["src"][0, :3].tolist() == [0, 4, 5]
    c["labels"][1, 0, 0] = 80
    assert _merge(c, 80, 0.5, 10000, 100)["src"][0, :2].tolist() == [0, 5]
    # a view that tripped: -1 and no rows
    c["counts"][0, 0] = -1
    out = _merge(c, 80, 0.5, 10000, 100)
    assert out["count"].tolist() == [-1] and bool((out["src"] == -1).all()) and _brute(c, 80, 0.5, 10000, 100) == [-1]


def test_flipping_twice_is_the_identity():
    img = np.random.default_rng(0).integers(0, 256, (2, 5, 7, 3), dtype=np.uint8)
    for d, name in ((1, "horizontal"), (2, "vertical"), (3, "diagonal")):
        f = R.flip(img, d)
        assert np.array_equal(f, R.flip(img, name)) and not np.array_equal(f, img) and np.array_equal(R.flip(f, d), img)
        assert np.array_equal(f[..., 0], R.flip(img, d)[..., 0])                # channels in place
    assert np.array_equal(R.flip(img, 1), img[:, :, ::-1]) and np.array_equal(R.flip(img, 2), img[:, ::-1])
    assert np.array_equal(R.flip(img, 3), img[:, ::-1, ::-1])
    b = np.asarray([[10.5, 50, 110.25, 90]], np.float32)
    for code in (0, 1, 2, 3):
        assert np.array_equal(R.unflip_boxes(R.unflip_boxes(b, code, 641, 427), code, 641, 427), b)


# -------------------------------------------------------------------------------------------------------------- plumbing
def test_test_time_aug_product_order_and_output_shape():
    from wedetect_amd.registry import TRANSFORMS
    from wedetect_amd.tta import TestTimeAug

    class Mark:
        def __init__(self, tag):
            self.tag = tag

        def __call__(self, r):
            r["trace"] = r.get("trace", []) + [self.tag]
            return r

    class Pack:
        def __call__(self, r):
            return dict(inputs=tuple(r["trace"]), data_samples=dict(r))

    t = TestTimeAug(transforms=[[Mark("a0"), Mark("a1")], [Mark("b0"), Mark("b1"), Mark("b2")], [Pack()]])
    src = dict(trace=["in"], other=[1, 2])
    out = t(src)
    assert sorted(out) == ["data_samples", "inputs"] and len(out["inputs"]) == len(out["data_samples"]) == 6
    assert out["inputs"] == [("in", a, b) for a in ("a0", "a1") for b in ("b0", "b1", "b2")]      # mmcv: first list outermost
    assert src == dict(trace=["in"], other=[1, 2])           # every branch ran on a copy
    assert TRANSFORMS.get("TestTimeAug") is TestTimeAug
    with pytest.raises(ValueError):
        TestTimeAug(transforms=[[], [Pack()]])
    built = TRANSFORMS.build(dict(type="TestTimeAug", transforms=[[dict(type="RandomFlip", prob=1.0), dict(type="RandomFlip", prob=0.0)],
                                                                  [dict(type="PackDetInputs", meta_keys=("flip", "flip_direction"))]]))
    assert len(built.subroutines) == 2 and [type(x).__name__ for x in built.subroutines[0].transforms] == ["RandomFlip", "PackDetInputs"]
    assert built.subroutines[0].transforms[0].prob == 1.0 and built.subroutines[1].transforms[0].prob == 0.0


def test_random_flip_refuses_a_random_flip():
    from wedetect_amd.tta import RandomFlip
    for bad in (0.5, None, [0.5], True):
        with pytest.raises(NotImplementedError):
            RandomFlip(prob=bad)
    with pytest.raises(ValueError):
        RandomFlip(prob=1.0, direction="sideways")
    r = RandomFlip(prob=0.0)(dict(img="untouched", pad_param=7))
    assert r == dict(img="untouched", pad_param=7, flip=False, flip_direction=None)
    assert RandomFlip(prob=1).direction == "horizontal" and RandomFlip(prob=1.0, direction="diagonal").prob == 1.0


def test_tta_cfg_and_collate():
    import torch
    from wedetect_amd import build as wb
    wb.build(verbose=False)
    from wedetect_amd.registry import MODELS
    from wedetect_amd.tta import DetTTAModel, check_tta_cfg, collate_views
    ok = dict(nms=dict(type="nms", iou_threshold=0.5), max_per_img=100)
    assert check_tta_cfg(ok) == ok
    assert check_tta_cfg(dict(nms=dict(type="nms", iou_threshold=0.6, split_thr=100), max_per_img=1024))["nms"]["split_thr"] == 100
    for bad in (dict(nms=dict(type="soft_nms", iou_threshold=0.5), max_per_img=100), dict(nms=dict(type="nms", iou_threshold=0.5), max_per_img=0),
                dict(nms=dict(type="nms", iou_threshold=0.5), max_per_img=1025), dict(nms=dict(type="nms"), max_per_img=100),
                dict(max_per_img=100), None, dict(nms=dict(type="nms", iou_threshold=0.5), max_per_img=100, score_thr=0.1)):
        with pytest.raises(NotImplementedError):
            check_tta_cfg(bad)
    assert MODELS.get("DetTTAModel") is DetTTAModel

    class Module:
        def predict_views(self, views, tta_cfg, stats=None):
            return [(len(views), [tuple(x.shape) for x, _ in views], [s for _, s in views], tta_cfg)]

    m = DetTTAModel(module=Module(), tta_cfg=ok)
    with pytest.raises(NotImplementedError):
        DetTTAModel(module=Module(), tta_cfg=dict(ok, max_per_img=2000))
    with pytest.raises(NotImplementedError):
        DetTTAModel(module=object(), tta_cfg=ok)
    items = [dict(inputs=[torch.full((3, 2, 2), 10 * i + v) for v in range(2)], data_samples=[f"s{i}v{v}" for v in range(2)]) for i in range(3)]
    data = collate_views(items)
    assert [tuple(x.shape) for x in data["inputs"]] == [(3, 3, 2, 2)] * 2 and int(data["inputs"][1][2, 0, 0, 0]) == 21
    assert data["data_samples"] == [["s0v0", "s1v0", "s2v0"], ["s0v1", "s1v1", "s2v1"]]
    (n, shapes, samples, cfg), = m.test_step(data)
    assert n == 2 and shapes == [(3, 3, 2, 2)] * 2 and samples == data["data_samples"] and cfg == ok
    with pytest.raises(ValueError):
        collate_views([items[0], dict(inputs=items[1]["inputs"][:1], data_samples=items[1]["data_samples"][:1])])


# --------------------------------------------------------------------------------------------------------------- test.py
def test_default_aug_test_pipeline_keeps_the_test_pipelines_meta_keys():
    import warnings
    from wedetect_amd.cfgfile import Config
    from wedetect_amd.pipeline import Compose
    T = _entry()
    cfg = Config.fromfile(os.path.join(ROOT, "config", "wedetect_tiny.py"))
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        tta_model, pipe = T.build_tta(cfg)
    assert len([x for x in w if "we will set it as default" in str(x.message)]) == 2
    assert tta_model == dict(type="DetTTAModel", tta_cfg=dict(nms=dict(type="nms", iou_threshold=0.5), max_per_img=100))
    test_pipe = list(cfg.test_pipeline)
    assert len(pipe) == len(test_pipe) and [dict(p)["type"] for p in pipe[:-1]] == [dict(p)["type"] for p in test_pipe[:-1]]
    last = pipe[-1]
    assert last["type"] == "TestTimeAug" and len(last["transforms"]) == 2
    assert [dict(t) for t in last["transforms"][0]] == [dict(type="RandomFlip", prob=1.0), dict(type="RandomFlip", prob=0.0)]
    (pack,) = last["transforms"][1]
    keys = tuple(pack["meta_keys"])
    own = tuple(test_pipe[-1]["meta_keys"])
    assert pack["type"] == "PackDetInputs" and keys[:len(own)] == own and keys[len(own):] == ("flip", "flip_direction")
    assert "pad_param" in keys and "texts" in keys
    assert test_pipe[-1]["type"] == "PackDetInputs" and "flip" not in test_pipe[-1]["meta_keys"]      # the config is not modified
    built = Compose(pipe)
    assert type(built.transforms[-1]).__name__ == "TestTimeAug" and len(built.transforms[-1].subroutines) == 2
    # a config's own tta_model / tta_pipeline are honoured
    cfg.tta_model = dict(type="DetTTAModel", tta_cfg=dict(nms=dict(type="nms", iou_threshold=0.6), max_per_img=300))
    cfg.tta_pipeline = [dict(type="LoadImageFromFile")]
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        tta_model, pipe = T.build_tta(cfg)
    assert not w and tta_model["tta_cfg"]["max_per_img"] == 300 and [dict(p) for p in pipe] == [dict(type="LoadImageFromFile")]


def test_test_py_flags(capsys):
    T = _entry()
    with pytest.raises(SystemExit) as e:
        T.parse_args(["c.py", "k.pth", "--tta"])
    assert e.value.code == 2 and "not implemented" in capsys.readouterr().err
    assert T.parse_args(["c.py", "k.pth"]).aug_test is False
    a = T.parse_args(["c.py", "k.pth", "--aug-test"])
    assert a.aug_test is True and a.loader == "serial"
    with pytest.raises(SystemExit) as e:
        T.parse_args(["c.py", "k.pth", "--aug-test", "--loader", "stream"])
    assert e.value.code == 2 and "--loader serial" in capsys.readouterr().err
    sh = open(os.path.join(ROOT, "dist_test.sh")).read()
    assert '--launcher pytorch "$@"' in sh                   # every test.py option, --aug-test included, passes through


# --------------------------------------------------------------------------------------------------- library and header
def test_library_exports_the_views_header_and_the_frozen_abi_is_untouched():
    from wedetect_amd import build as wb
    wb.build(verbose=False)
    decl = set(declared(VIEWS_HEADER))
    assert {"wd_views_abi_version", "wd_flip_u8", "wd_views_merge", "wd_views_merge_workspace_bytes"} == decl
    lib = ctypes.CDLL(wb.LIB)
    assert not [s for s in sorted(decl) if not hasattr(lib, s)]
    from wedetect_amd import feed as F
    from wedetect_amd import lib as L
    from wedetect_amd import tile as T
    from wedetect_amd import views as VW
    assert set(VW.EXPORTS) == decl
    assert not set(VW.EXPORTS) & (set(L.EXPORTS) | set(F.EXPORTS) | set(T.EXPORTS))
    assert VW.LIB.wd_views_abi_version() == VW.VIEWS_ABI_VERSION == 1
    assert L.LIB.wd_abi_version() == L.ABI_VERSION == 15 and T.LIB.wd_tile_abi_version() == 1
    assert hashlib.sha256(open(os.path.join(ROOT, "include", "wedetect_hip.h"), "rb").read()).hexdigest() == MAIN_HEADER_SHA256
    assert "views.hip" in wb.SOURCES and "wedetect_hip_views.h" in wb.PUBLIC_HEADERS
    assert set(wb.NO_SCRATCH["views.hip"]) == {"flip_u8_kernel", "views_sort_kernel"} and wb.ASM_VMEM_SOURCES["views.hip"] == []
    # the limits, refused before any launch (no device needed: the checks come first)
    assert VW.merge_workspace_bytes(8, 65535, 512) > VW.merge_workspace_bytes(2, 32, 300) > 0
    assert 0 == VW.merge_workspace_bytes(9, 1, 4) == VW.merge_workspace_bytes(8, 1, 513) == VW.merge_workspace_bytes(0, 1, 5)
    assert 0 == VW.merge_workspace_bytes(2, 65536, 4) == VW.merge_workspace_bytes(2, 0, 4)
    one = ctypes.c_void_p(256)                               # non-null, aligned, never dereferenced: refused first
    call = lambda V, B, max_in, n_cls, max_out, thr=0.5, ws=1 << 40, p=one: VW.LIB.wd_views_merge(
        p, one, one, one, one, one, V, B, max_in, n_cls, thr, 10000, max_out, one, one, one, one, one, one, ws, None)
    assert call(9, 1, 4, 80, 300) == -4 and call(0, 1, 4, 80, 300) == -4
    assert call(8, 1, 513, 80, 300) == -4 and call(2, 32, 300, 80, 1025) == -4 and call(8, 1, 512, 1 << 19, 300) == -4
    assert call(2, 0, 300, 80, 300) == -1 and call(2, 65536, 300, 80, 300) == -1 and call(2, 32, 0, 80, 300) == -1
    assert call(2, 32, 300, 0, 300) == -1 and call(2, 32, 300, 80, 0) == -1
    assert call(2, 32, 300, 80, 300, float("nan")) == -1 and call(2, 32, 300, 80, 300, float("inf")) == -1
    assert call(2, 32, 300, 80, 300, p=None) == -1 and call(2, 32, 300, 80, 300, p=ctypes.c_void_p(264)) == -1      # null, misaligned boxes
    assert call(2, 32, 300, 80, 300, ws=VW.merge_workspace_bytes(2, 32, 300) - 1) == -3
    flip = lambda s, d, n, h, w, direction: VW.LIB.wd_flip_u8(s, d, n, h, w, direction, None)
    a, b = ctypes.c_void_p(4096), ctypes.c_void_p(4096 + 2 * 3 * 5 * 3)
    assert flip(None, b, 2, 3, 5, 1) == -1 and flip(a, None, 2, 3, 5, 1) == -1
    assert flip(a, b, 2, 3, 5, 0) == -1 and flip(a, b, 2, 3, 5, 4) == -1 and flip(a, b, 0, 3, 5, 1) == -1 and flip(a, b, 2, 0, 5, 1) == -1
    assert flip(a, b, 2, 3, 0, 1) == -1 and flip(a, b, 65536, 3, 5, 1) == -1
    assert flip(a, a, 2, 3, 5, 1) == -1 and flip(a, ctypes.c_void_p(4096 + 89), 2, 3, 5, 1) == -1 and flip(b, a, 2, 3, 6, 1) == -1      # overlap


def test_every_views_entry_point_with_device_memory_has_an_extents_case():
    from tests.test_cpu_arena import EXEMPT_ALLOWED, _takes_memory
    from tests.test_gpu_views_extents import CASES, EXEMPT
    decl = declared(VIEWS_HEADER)
    covered = {c.entry for c in CASES}
    allowed = EXEMPT_ALLOWED + ("wd_views_abi_version",)
    for name in sorted(decl):
        assert name in covered or name in EXEMPT, f"{name}: views entry without a case in tests/test_gpu_views_extents.py (or an EXEMPT reason)"
        assert not (name in covered and name in EXEMPT), f"{name}: both covered and exempt"
    for name, reason in EXEMPT.items():
        assert name in decl, f"EXEMPT names {name}, which the header does not declare"
        assert isinstance(reason, str) and reason.strip() and "\n" not in reason
        assert any(fnmatch.fnmatch(name, pat) for pat in allowed), f"{name} may not be exempt: it must have a case"
        assert not _takes_memory(decl[name]), f"{name} takes device memory: it must have a case"
    for name in ("wd_flip_u8", "wd_views_merge"):
        assert _takes_memory(decl[name]) and name in covered
    assert not covered - set(decl)
    ids = [c.id for c in CASES]
    assert len(ids) == len(set(ids))
