"""Guard-band tests (GPU) of include/wedetect_hip_tile.h, run as tests/test_gpu_extents.py runs the entry points of the main
header (same harness: its Ctx / Run / Case / execute): every operand of ``wd_tile_cut_u8`` and ``wd_tile_merge`` is carved from
a tests/arena.py Arena with guard bands, the case runs in 0x00 and in 0xFF surroundings (outputs bit-identical), inputs stay
unchanged, the merge's workspace starts as 0xFF bytes (and as zeros: same bits; a second launch on the dirty workspace: same
bits), and the outputs — which start out holding the pattern — equal the reference in every element.

The bytes between two rows of a padded-pitch source image hold the arena's pattern, and so does the overview slot of the cut's
destination, which must still hold it afterwards.

tests/test_cpu_tile.py asserts on the CPU that every function of the tile header that takes device memory has a case here.
"""
from __future__ import annotations

from typing import List

import numpy as np
import pytest
import torch

import tests.test_gpu_extents as X
from tests import tile_ref as R

pytestmark = pytest.mark.gpu

u8, i32, f32 = torch.uint8, torch.int32, torch.float32

CASES: List[X.Case] = []

EXEMPT = {
    "wd_tile_abi_version": "no memory",
    "wd_tile_sizeof_tile": "no memory",
    "wd_tile_merge_workspace_bytes": "size query, no memory",
}


def case(entry: str, name: str, cap: int = 64 << 20, **kw):
    def deco(fn):
        CASES.append(X.Case(entry, name, (lambda ctx, _fn=fn, _kw=kw: _fn(ctx, **_kw)), cap))
        return fn
    return deco


@case("wd_tile_cut_u8", "70x101 -> 32x32 tiles, dense rows at an odd address, dword stores", hw=(70, 101), tile=(32, 32), overlap=0.25, pad=0, swap=0)
@case("wd_tile_cut_u8", "70x101 -> 64x96 tiles, pitch + 13, swapped, dst at an odd address (byte stores)", hw=(70, 101), tile=(64, 96), overlap=0.2, pad=13, swap=1, dst_mis=1)
@case("wd_tile_cut_u8", "20x50 in a 32x64 tile (fill), pitch + 2", hw=(20, 50), tile=(32, 64), overlap=0.2, pad=2, swap=0)
@case("wd_tile_cut_u8", "crops + overview slot (untouched) + blank tiles", hw=(70, 101), tile=(32, 32), overlap=0.25, pad=7, swap=1, extra=True)
def _cut(ctx, hw, tile, overlap, pad, swap, dst_mis=4, extra=False):
    from wedetect_amd import tile as T, tiling as G
    h, w = hw
    th, tw = tile
    img = np.random.default_rng(h * w + pad).integers(0, 256, (h, w, 3), dtype=np.uint8)
    plan = G.plan_tiles(h, w, tile, overlap, overview=extra)
    if extra:
        plan = G.pad_plan(plan, len(plan) + 2)
    n = len(plan)
    pitch = w * 3 + pad
    src = ctx.inp("img", torch.from_numpy(img.reshape(h, w * 3).copy()), ld=pitch, mis=1)
    dd = ctx.inp("tiles", torch.from_numpy(plan.view(np.uint8).copy()), mis=4)
    dst = ctx.out("dst", (n * th, tw * 3), u8, mis=dst_mis)
    written = torch.from_numpy(np.repeat(plan["kind"] != G.OVERVIEW, th)).to(dst.device)
    pattern = ctx.ar.pattern

    def launch():
        ctx.L.check(T.LIB.wd_tile_cut_u8(src.data_ptr(), h, w, pitch, dd.data_ptr(), plan.ctypes.data, n, th, tw, 114, swap,
                                         dst.data_ptr(), ctx.L.stream_ptr()), "wd_tile_cut_u8")

    def value(o):
        assert bool((dst[~written] == pattern).all()), "the overview slot was written"
        want = R.cut(img, plan, tile, 114, bool(swap))[plan["kind"] != G.OVERVIEW]
        got = o["dst"].cpu().numpy().reshape(-1, th, tw, 3)
        assert np.array_equal(got, want), f"{int((got != want).sum())} bytes differ"
    return X.Run(launch, lambda: {"dst": dst[written]}, value, f"{n} tiles of {th}x{tw}, pitch {pitch}")


@case("wd_tile_merge", "1 x 5", n_tile=1, max_in=5, margin=0.0, split_thr=10000, max_out=300)
@case("wd_tile_merge", "3 x 64, margin 2, max_out 7", n_tile=3, max_in=64, margin=2.0, split_thr=10000, max_out=7)
@case("wd_tile_merge", "9 x 300, margin 2, per class", n_tile=9, max_in=300, margin=2.0, split_thr=8, max_out=300)
@case("wd_tile_merge", "128 x 256 (the cap: four sort chunks), blank tiles", n_tile=128, max_in=256, margin=2.0, split_thr=10000, max_out=1024)
def _merge(ctx, n_tile, max_in, margin, split_thr, max_out):
    from wedetect_amd import tile as T
    L = ctx.L
    c = R.merge_inputs(n_tile, max_in, seed=n_tile)
    t = torch.from_numpy
    boxes = ctx.inp("boxes", t(c["boxes"].reshape(n_tile * max_in, 4)), mis=16)
    scores = ctx.inp("scores", t(c["scores"].reshape(1, -1)), mis=4)
    labels = ctx.inp("labels", t(c["labels"].reshape(1, -1)), mis=4)
    counts = ctx.inp("counts", t(c["counts"].reshape(1, -1)), mis=4)
    dd = ctx.inp("tiles", t(c["plan"].view(np.uint8).copy()), mis=4)
    ob = ctx.out("out_boxes", (max_out, 4), f32, mis=16)
    os_ = ctx.out("out_scores", (1, max_out), f32, mis=4)
    ol = ctx.out("out_labels", (1, max_out), i32, mis=4, fillers=(-1,))
    osrc = ctx.out("out_src", (1, max_out), i32, mis=4, fillers=(-1,))
    oc = ctx.out("out_count", (1, 1), i32, mis=4, fillers=(-1,))
    nbytes = T.merge_workspace_bytes(n_tile, max_in)
    ws = ctx.ws("workspace", nbytes, mis=0)
    thr = L.nms_threshold(0.7, L.NMS_MMCV)

    def launch():
        L.check(T.LIB.wd_tile_merge(boxes.data_ptr(), scores.data_ptr(), labels.data_ptr(), counts.data_ptr(), dd.data_ptr(), n_tile,
                                    max_in, R.N_CLS, margin, thr, split_thr, max_out, ob.data_ptr(), os_.data_ptr(), ol.data_ptr(),
                                    osrc.data_ptr(), oc.data_ptr(), ws.data_ptr(), nbytes, L.stream_ptr()), "wd_tile_merge")

    def value(o):
        want = R.merge(c["boxes"], c["scores"], c["labels"], c["counts"], c["plan"], R.N_CLS, margin, 0.7, split_thr, max_out)
        assert int(o["out_count"].item()) == want["count"] >= 1
        assert np.array_equal(o["out_src"].cpu().numpy().reshape(-1), want["src"])
        assert np.array_equal(o["out_labels"].cpu().numpy().reshape(-1), want["labels"])
        assert np.array_equal(o["out_scores"].cpu().numpy().reshape(-1).view(np.uint32), want["scores"].view(np.uint32))
        assert np.array_equal(o["out_boxes"].cpu().numpy().view(np.uint32), want["boxes"].view(np.uint32))
    return X.Run(launch, lambda: {"out_boxes": ob, "out_scores": os_, "out_labels": ol, "out_src": osrc, "out_count": oc}, value,
                 f"{n_tile} x {max_in} rows, workspace {nbytes} bytes")


@pytest.mark.parametrize("c", CASES, ids=[c.id for c in CASES])
def test_tile_extents(c):
    run0, o0, _ = X.execute(c, 0x00, 0xFF)
    run1, o1, _ = X.execute(c, 0xFF, 0xFF)
    X._same(o0, o1, "surroundings 0x00 vs 0xFF")
    for k, v in o1.items():
        if v.dtype.is_floating_point:
            assert bool(torch.isfinite(v).all()), f"output {k!r}: non-finite element(s)"
    if run0.has_ws:
        _, o2, _ = X.execute(c, 0x00, 0x00)
        X._same(o0, o2, "workspace 0xFF vs zero-filled")
    run0.value(o0)
    print(f"{c.id}: {run0.info}: guards clean, 0x00 == 0xFF" + (", workspace hygiene ok" if run0.has_ws else ""))
