"""Tiled inference without a GPU: the tile plan, the tile header and its binding, the coverage rule of the extent tests applied
to the new header, tests/tile_ref.py against a brute-force loop, and the demo's new flags."""
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

from tests import tile_ref as R  # noqa: E402
from tests.abi_decl import declared  # noqa: E402
from wedetect_amd import tiling as G  # noqa: E402

TILE_HEADER = "wedetect_hip_tile.h"
# sha256 of include/wedetect_hip.h at ABI 15 (tests/test_cpu_feed.py pins the same): the tile entry points live in a header of
# their own, the frozen one does not move
MAIN_HEADER_SHA256 = "2b62a824664907f02d66fef8abe43f4c50fa0703c00814e15a08129143937784"


# ------------------------------------------------------------------------------------------------------------------ plan
def _covered(plan, h, w):
    seen = np.zeros((h, w), np.int32)
    for t in plan[plan["kind"] == G.CROP]:
        assert t["x0"] >= 0 and t["y0"] >= 0 and t["x0"] + t["w"] <= w and t["y0"] + t["h"] <= h      # inside the image
        assert t["w"] >= 1 and t["h"] >= 1
        seen[t["y0"]:t["y0"] + t["h"], t["x0"]:t["x0"] + t["w"]] += 1
    return seen


PLANS = [
    # (h, w), tile, overlap -> x origins, y origins
    ((70, 101), (32, 32), 0.25, [0, 24, 48, 69], [0, 24, 38]),
    ((96, 160), (64, 64), 0.5, [0, 32, 64, 96], [0, 32]),
    ((2160, 3840), (640, 640), 0.2, [0, 512, 1024, 1536, 2048, 2560, 3072, 3200], [0, 512, 1024, 1520]),
    ((20, 50), (32, 64), 0.2, [0], [0]),
    ((70, 101), (32, 32), 0.0, [0, 32, 64, 69], [0, 32, 38]),
    ((64, 65), (64, 64), 0.5, [0, 1], [0]),
]


@pytest.mark.parametrize("hw,tile,overlap,xs,ys", PLANS, ids=[f"{p[0][0]}x{p[0][1]} tile {p[1][0]}x{p[1][1]} overlap {p[2]}" for p in PLANS])
def test_plan_counts_origins_and_coverage(hw, tile, overlap, xs, ys):
    h, w = hw
    plan = G.plan_tiles(h, w, tile, overlap, overview=False)
    assert plan.dtype == G.TILE_DTYPE and plan.dtype.itemsize == 32
    assert len(plan) == len(xs) * len(ys) == G.n_crops(plan)
    assert plan["x0"].tolist() == xs * len(ys)                                   # row-major
    assert plan["y0"].tolist() == [y for y in ys for _ in xs]
    assert bool((_covered(plan, h, w) >= 1).all())                               # every pixel lies in at least one crop
    assert bool((plan["img_w"] == w).all()) and bool((plan["img_h"] == h).all())
    th, tw = tile
    assert set(plan["w"].tolist()) == {min(w, tw)} and set(plan["h"].tolist()) == {min(h, th)}      # every tile is full
    for t in plan:
        want = 1 * (t["x0"] > 0) | 2 * (t["y0"] > 0) | 4 * (t["x0"] + t["w"] < w) | 8 * (t["y0"] + t["h"] < h)
        assert t["interior_mask"] == want
    assert plan.tobytes() == G.plan_tiles(h, w, tile, overlap, overview=False).tobytes()              # deterministic
    with_ov = G.plan_tiles(h, w, tile, overlap, overview=True)
    if len(plan) > 1:
        assert len(with_ov) == len(plan) + 1 and with_ov[:-1].tobytes() == plan.tobytes()
        o = with_ov[-1]
        assert (o["kind"], o["x0"], o["y0"], o["w"], o["h"], o["interior_mask"]) == (G.OVERVIEW, 0, 0, w, h, 0)
        assert not G.fits_one_tile(with_ov)
    else:
        assert with_ov.tobytes() == plan.tobytes() and G.fits_one_tile(with_ov)   # the caller runs plain predict


def test_plan_masks_on_corner_edge_and_inner_tiles():
    plan = G.plan_tiles(2160, 3840, (640, 640), 0.2)
    assert len(plan) == 33 and G.n_crops(plan) == 32
    m = plan["interior_mask"][:32].reshape(4, 8)
    L_, T_, R_, B_ = G.LEFT, G.TOP, G.RIGHT, G.BOTTOM
    assert m[0, 0] == R_ | B_ and m[0, 7] == L_ | B_ and m[3, 0] == R_ | T_ and m[3, 7] == L_ | T_          # corners
    assert m[0, 3] == L_ | R_ | B_ and m[3, 3] == L_ | R_ | T_ and m[1, 0] == T_ | B_ | R_ and m[2, 7] == T_ | B_ | L_   # edges
    assert bool((m[1:3, 1:7] == 15).all())                                                                   # inner
    assert G.step_sizes(33, 32) == [(32, 32), (1, 1)] and G.step_sizes(9, 4) == [(4, 4), (4, 4), (1, 1)]
    assert G.step_sizes(8, 5) == [(5, 5), (3, 4)] and G.step_sizes(21, 32) == [(21, 32)] and G.step_sizes(64, 32) == [(32, 32)] * 2
    padded = G.pad_plan(plan, 40)
    assert padded[:33].tobytes() == plan.tobytes() and set(padded["kind"][33:].tolist()) == {G.BLANK}
    meta = G.tile_meta(padded, (640, 640), overview_meta=[1, 2, 0, .5, .5, 3840, 2160, 1])
    assert meta[0].tolist() == [0, 0, 0, 1, 1, 640, 640, 1] and meta[32].tolist() == [1, 2, 0, .5, .5, 3840, 2160, 1]


def test_plan_refuses_bad_arguments():
    for bad in (dict(tile=(63, 64)), dict(tile=(0, 64)), dict(overlap=0.6), dict(overlap=-0.1), dict(tile=64)):
        with pytest.raises((ValueError, TypeError)):
            G.plan_tiles(100, 100, **{"tile": (64, 64), "overlap": 0.2, **bad})
    with pytest.raises(ValueError):
        G.plan_tiles(0, 10)


def test_overview_geometry_is_the_test_pipelines_own():
    from wedetect_amd.preprocess import mmdet_test_geometry
    for (h, w), tile in (((2160, 3840), (640, 640)), ((96, 160), (64, 64)), ((70, 101), (64, 96))):
        g = G.overview_geometry(h, w, tile)
        ref = mmdet_test_geometry(h, w, (tile[1], tile[0]))
        assert np.array_equal(g["pad_param"], ref["pad_param"]) and tuple(g["scale_factor"]) == tuple(ref["scale_factor"])
        assert (g["dh"], g["dw"]) == ref["no_pad_shape"] and g["canvas"] == tile and g["pad_val"] == 114
        assert g["meta"][:2] == [float(ref["pad_param"][2]), float(ref["pad_param"][0])] and g["meta"][5:] == [float(w), float(h), 1.0]


# --------------------------------------------------------------------------------------------------- library and header
def test_library_exports_the_tile_header_and_the_frozen_abi_is_untouched():
    from wedetect_amd import build as wb
    wb.build(verbose=False)
    decl = set(declared(TILE_HEADER))
    assert {"wd_tile_abi_version", "wd_tile_sizeof_tile", "wd_tile_cut_u8", "wd_tile_merge", "wd_tile_merge_workspace_bytes"} == decl
    lib = ctypes.CDLL(wb.LIB)
    assert not [s for s in sorted(decl) if not hasattr(lib, s)]
    from wedetect_amd import feed as F
    from wedetect_amd import lib as L
    from wedetect_amd import tile as T
    assert set(T.EXPORTS) == decl
    assert not set(T.EXPORTS) & set(L.EXPORTS) and not set(T.EXPORTS) & set(F.EXPORTS)
    assert T.LIB.wd_tile_abi_version() == T.TILE_ABI_VERSION == 1
    assert T.LIB.wd_tile_sizeof_tile() == ctypes.sizeof(T.Tile) == G.TILE_DTYPE.itemsize == 32
    for f, _ in T.Tile._fields_:                             # the numpy view of a descriptor is the C struct
        assert G.TILE_DTYPE.fields[f][1] == getattr(T.Tile, f).offset, f
    assert L.LIB.wd_abi_version() == L.ABI_VERSION == 15
    assert hashlib.sha256(open(os.path.join(ROOT, "include", "wedetect_hip.h"), "rb").read()).hexdigest() == MAIN_HEADER_SHA256
    assert "tile.hip" in wb.SOURCES and "wedetect_hip_tile.h" in wb.PUBLIC_HEADERS
    assert set(wb.NO_SCRATCH["tile.hip"]) == {"tile_cut_kernel", "merge_keys_kernel"}
    # the merge's limits, refused before any launch (no device needed: the checks come first)
    assert T.merge_workspace_bytes(128, 256) > 0 == T.merge_workspace_bytes(129, 256) == T.merge_workspace_bytes(0, 5)
    one = ctypes.c_void_p(256)                               # non-null, aligned, never dereferenced: refused first
    call = lambda n_tile, max_in, n_cls, max_out: T.LIB.wd_tile_merge(one, one, one, one, one, n_tile, max_in, n_cls, 2.0, 0.7, 10000,
                                                                      max_out, one, one, one, one, one, one, 1 << 30, None)
    assert call(129, 256, 80, 300) == -4 and call(128, 256, 80, 1025) == -4 and call(128, 256, 65536, 300) == -4
    assert call(0, 256, 80, 300) == -1


def test_every_tile_entry_point_with_device_memory_has_an_extents_case():
    from tests.test_cpu_arena import EXEMPT_ALLOWED, _takes_memory
    from tests.test_gpu_tile_extents import CASES, EXEMPT
    decl = declared(TILE_HEADER)
    covered = {c.entry for c in CASES}
    allowed = EXEMPT_ALLOWED + ("wd_tile_abi_version", "wd_tile_sizeof_*")
    for name in sorted(decl):
        assert name in covered or name in EXEMPT, f"{name}: tile entry without a case in tests/test_gpu_tile_extents.py (or an EXEMPT reason)"
        assert not (name in covered and name in EXEMPT), f"{name}: both covered and exempt"
    for name, reason in EXEMPT.items():
        assert name in decl, f"EXEMPT names {name}, which the header does not declare"
        assert isinstance(reason, str) and reason.strip() and "\n" not in reason
        assert any(fnmatch.fnmatch(name, pat) for pat in allowed), f"{name} may not be exempt: it must have a case"
        assert not _takes_memory(decl[name]), f"{name} takes device memory: it must have a case"
    for name in ("wd_tile_cut_u8", "wd_tile_merge"):
        assert _takes_memory(decl[name]) and name in covered
    assert not covered - set(decl)
    ids = [c.id for c in CASES]
    assert len(ids) == len(set(ids))


# -------------------------------------------------------------------------------------------------------------- tile_ref
def _plan2():
    """Two 64 x 64 crops side by side (overlap 16 pixels) + the overview of the 64 x 112 image."""
    plan = G.plan_tiles(64, 112, (64, 64), 0.25)
    assert plan["x0"].tolist() == [0, 48, 0] and plan["interior_mask"].tolist() == [G.RIGHT, G.LEFT, 0]
    return plan


def test_tile_ref_merge_on_hand_made_vectors():
    plan = _plan2()
    nan = np.float32("nan")
    boxes = np.full((3, 4, 4), nan, np.float32)
    scores = np.full((3, 4), nan, np.float32)
    labels = np.full((3, 4), 2 ** 30, np.int32)
    # crop 0: A whole inside, B touching the interior (right) side -> dropped at margin 2, C in the overlap
    boxes[0, :3] = [[5, 5, 20, 20], [50, 10, 64, 30], [50, 40, 60, 50]]
    scores[0, :3] = [0.9, 0.8, 0.5]
    labels[0, :3] = [1, 1, 0]
    # crop 1: C again (image x 50..60 = local 2..12, score higher: it wins), D starting at the interior (left) side -> dropped,
    # E at the image's right side (no interior side there) -> kept, and a row BEYOND the count that must not matter
    boxes[1, :4] = [[2, 40, 12, 50], [0, 5, 9, 20], [50, 5, 64, 20], [2, 40, 12, 50]]
    scores[1, :4] = [0.6, 0.7, 0.5, 0.99]
    labels[1, :4] = [0, 3, 3, 0]
    # overview (image pixels): A again with a lower score -> suppressed by crop 0's row; F on its own, a different class over C
    boxes[2, :3] = [[5, 5, 20, 20.5], [70, 30, 100, 60], [50, 40, 60, 50]]
    scores[2, :3] = [0.85, 0.5, 0.4]
    labels[2, :3] = [1, 2, 7]
    counts = np.asarray([3, 3, 3], np.int32)
    out = R.merge(boxes, scores, labels, counts, plan, 80, 2.0, 0.7, 10000, 300)
    k = out["count"]
    # (score desc, slot asc): A 0.9, C(crop 1) 0.6, E 0.5 (slot 6), F 0.5 (slot 9), C-as-class-7 0.4
    assert out["src"][:k].tolist() == [0, 4, 6, 9, 10] and out["labels"][:k].tolist() == [1, 0, 3, 2, 7]
    assert out["boxes"][:k].tolist() == [[5, 5, 20, 20], [50, 40, 60, 50], [98, 5, 112, 20], [70, 30, 100, 60], [50, 40, 60, 50]]
    assert out["dropped"] == 2 and out["cross_tile"] == 2
    assert bool((out["src"][k:] == -1).all()) and bool((out["labels"][k:] == -1).all()) and not out["boxes"][k:].any()
    assert R.merge_brute(boxes, scores, labels, counts, plan, 80, 2.0, 0.7, 300) == list(zip(out["src"][:k].tolist(), out["labels"][:k].tolist()))
    # margin 0: B and D stay
    out0 = R.merge(boxes, scores, labels, counts, plan, 80, 0.0, 0.7, 10000, 300)
    assert out0["dropped"] == 0 and sorted(out0["src"][:out0["count"]].tolist()) == [0, 1, 4, 5, 6, 9, 10]
    # max_out below the survivor count: the prefix
    out3 = R.merge(boxes, scores, labels, counts, plan, 80, 2.0, 0.7, 10000, 3)
    assert out3["count"] == 3 and out3["src"].tolist() == [0, 4, 6]
    # per-class branch (split_thr below the candidate count): the same rows here
    outc = R.merge(boxes, scores, labels, counts, plan, 80, 2.0, 0.7, 2, 300)
    assert outc["src"][:k].tolist() == out["src"][:k].tolist()
    # a tile that tripped; a blank tile's count is not read
    bad = counts.copy()
    bad[1] = -1
    assert R.merge(boxes, scores, labels, bad, plan, 80, 2.0, 0.7, 10000, 300)["count"] == -1
    blank = plan.copy()
    blank["kind"][1] = G.BLANK
    ob = R.merge(boxes, scores, labels, bad, blank, 80, 2.0, 0.7, 10000, 300)
    assert ob["src"][:ob["count"]].tolist() == [0, 2, 9, 10]


@pytest.mark.parametrize("n_tile,max_in,margin", [(1, 5, 0.0), (3, 64, 2.0), (3, 64, 0.0), (9, 300, 2.0)])
def test_tile_ref_merge_equals_the_brute_force_loop(n_tile, max_in, margin):
    """On the GPU tests' own inputs (planted IoUs are 1 and 0.6, far from the threshold 0.7 in fp32 and fp64 alike)."""
    c = R.merge_inputs(n_tile, max_in, seed=n_tile)
    out = R.merge(c["boxes"], c["scores"], c["labels"], c["counts"], c["plan"], R.N_CLS, margin, 0.7, 10000, 300)
    k = out["count"]
    brute = R.merge_brute(c["boxes"], c["scores"], c["labels"], c["counts"], c["plan"], R.N_CLS, margin, 0.7, 300)
    assert k >= 1 and [s for s, _ in brute] == out["src"][:k].tolist()
    assert bool((np.diff(out["scores"][:k]) <= 0).all())
    kinds = c["plan"]["kind"][out["src"][:k] // max_in]
    assert bool((kinds != G.BLANK).all())


def test_cut_reference_fill_blank_and_overview():
    img = np.random.default_rng(0).integers(0, 256, (20, 50, 3), dtype=np.uint8)
    plan = G.pad_plan(G.plan_tiles(20, 50, (32, 64)), 3)
    plan["kind"][1] = G.OVERVIEW
    dst = np.full((3, 32, 64, 3), 9, np.uint8)
    out = R.cut(img, plan, (32, 64), 114, swap_rb=True, dst=dst)
    assert np.array_equal(out[0, :20, :50], img[:, :, ::-1]) and bool((out[0, 20:] == 114).all()) and bool((out[0, :, 50:] == 114).all())
    assert bool((out[1] == 9).all()) and bool((out[2] == 114).all())


# ------------------------------------------------------------------------------------------------------------------ demo
def test_demo_takes_the_tile_flags_and_tiling_is_off_by_default():
    import infer_wedetect as I
    a = I.parse_args([])
    assert a.tile == 0 and a.tile_overlap == 0.2 and a.tile_batch == 32 and a.no_overview is False and a.edge_margin == 2.0
    a = I.parse_args(["--tile", "640", "--tile-overlap", "0.25", "--tile-batch", "16", "--no-overview", "--edge-margin", "0"])
    assert (a.tile, a.tile_overlap, a.tile_batch, a.no_overview, a.edge_margin) == (640, 0.25, 16, True, 0.0)
    from wedetect_amd.detector import YOLOWorldDetector
    import inspect
    sig = inspect.signature(YOLOWorldDetector.predict_tiled)
    d = {k: p.default for k, p in sig.parameters.items()}
    assert d["tile"] is None and d["overlap"] == 0.2 and d["overview"] is True and d["tile_batch"] == 32 and d["edge_margin"] == 2.0
    assert d["merge_iou"] is None and d["max_per_img"] is None and d["channel_order"] == "rgb" and d["texts"] is None
