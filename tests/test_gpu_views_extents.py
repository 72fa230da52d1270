"""Guard-band tests (GPU) of include/wedetect_hip_views.h, run as tests/test_gpu_extents.py runs the entry points of the main
header (same harness: its Ctx / Run / Case / execute): every operand of ``wd_flip_u8`` and ``wd_views_merge`` is carved from a
tests/arena.py Arena with guard bands, the case runs in 0x00 and in 0xFF surroundings (outputs bit-identical), inputs stay
unchanged, the merge's workspace starts as 0xFF bytes (and as zeros: same bits; a second launch on the dirty workspace: same
bits), and the outputs — which start out holding the pattern — equal the reference in every element.

tests/test_cpu_views.py asserts on the CPU that every function of the views header that takes device memory has a case here.
"""
from __future__ import annotations

from typing import List

import numpy as np
import pytest
import torch

import tests.test_gpu_extents as X
from tests import views_ref as R

pytestmark = pytest.mark.gpu

u8, i32, f32 = torch.uint8, torch.int32, torch.float32

CASES: List[X.Case] = []

EXEMPT = {
    "wd_views_abi_version": "no memory",
    "wd_views_merge_workspace_bytes": "size query, no memory",
}


def case(entry: str, name: str, cap: int = 64 << 20, **kw):
    def deco(fn):
        CASES.append(X.Case(entry, name, (lambda ctx, _fn=fn, _kw=kw: _fn(ctx, **_kw)), cap))
        return fn
    return deco


@case("wd_flip_u8", "2x3x5 horizontal, byte path (odd w)", shape=(2, 3, 5), direction=1)
@case("wd_flip_u8", "2x64x96 diagonal, dword path", shape=(2, 64, 96), direction=3, mis=4)
@case("wd_flip_u8", "2x64x96 vertical, dword path", shape=(2, 64, 96), direction=2, mis=4)
@case("wd_flip_u8", "3x32x33 horizontal, dst at an odd address", shape=(3, 32, 33), direction=1, mis=4, dst_mis=1)
@case("wd_flip_u8", "1x8x16 horizontal, w % 4 == 0 but src at an odd address (byte path)", shape=(1, 8, 16), direction=1, mis=1, dst_mis=4)
def _flip(ctx, shape, direction, mis=1, dst_mis=None):
    from wedetect_amd import views as VW
    n, h, w = shape
    img = np.random.default_rng(n * h * w + direction).integers(0, 256, (n, h, w, 3), dtype=np.uint8)
    src = ctx.inp("src", torch.from_numpy(img.reshape(n * h, w * 3).copy()), mis=mis)
    dst = ctx.out("dst", (n * h, w * 3), u8, mis=mis if dst_mis is None else dst_mis)

    def launch():
        ctx.L.check(VW.LIB.wd_flip_u8(src.data_ptr(), dst.data_ptr(), n, h, w, direction, ctx.L.stream_ptr()), "wd_flip_u8")

    def value(o):
        got = o["dst"].cpu().numpy().reshape(n, h, w, 3)
        want = R.flip(img, direction)
        assert np.array_equal(got, want), f"{int((got != want).sum())} bytes differ"
    return X.Run(launch, lambda: {"dst": dst}, value, f"{n} x {h} x {w}, direction {direction}, src % 4 = {src.data_ptr() % 4}, "
                                                       f"dst % 4 = {dst.data_ptr() % 4}")


@case("wd_views_merge", "1 x 1 x 5", V=1, B=1, max_in=5, counts="full", n_cls=1, split_thr=10000, max_out=300)
@case("wd_views_merge", "2 x 3 x 300 (the shipped shape)", V=2, B=3, max_in=300, counts="mixed", n_cls=80, split_thr=10000, max_out=300)
@case("wd_views_merge", "4 x 2 x 64, per class, max_out 7", V=4, B=2, max_in=64, counts="mixed", n_cls=80, split_thr=8, max_out=7)
def _merge(ctx, V, B, max_in, counts, n_cls, split_thr, max_out):
    from wedetect_amd import views as VW
    L = ctx.L
    c = R.merge_inputs(V, B, max_in, seed=V * 100 + B, counts=counts, n_cls=n_cls)
    t = torch.from_numpy
    boxes = ctx.inp("boxes", t(c["boxes"].reshape(V * B * max_in, 4)), mis=16)
    scores = ctx.inp("scores", t(c["scores"].reshape(1, -1)), mis=4)
    labels = ctx.inp("labels", t(c["labels"].reshape(1, -1)), mis=4)
    cnt = ctx.inp("counts", t(c["counts"].reshape(1, -1)), mis=4)
    vf = ctx.inp("view_flip", t(c["view_flip"].reshape(1, -1)), mis=4)
    wh = ctx.inp("img_wh", t(c["img_wh"].reshape(1, -1)), mis=4)
    ob = ctx.out("out_boxes", (B * max_out, 4), f32, mis=16)
    os_ = ctx.out("out_scores", (B, max_out), f32, mis=4)
    ol = ctx.out("out_labels", (B, max_out), i32, mis=4, fillers=(-1,))
    osrc = ctx.out("out_src", (B, max_out), i32, mis=4, fillers=(-1,))
    oc = ctx.out("out_count", (1, B), i32, mis=4, fillers=(-1,))
    nbytes = VW.merge_workspace_bytes(V, B, max_in)
    ws = ctx.ws("workspace", nbytes, mis=0)
    thr = L.nms_threshold(0.5, L.NMS_MMCV)

    def launch():
        L.check(VW.LIB.wd_views_merge(boxes.data_ptr(), scores.data_ptr(), labels.data_ptr(), cnt.data_ptr(), vf.data_ptr(), wh.data_ptr(),
                                      V, B, max_in, n_cls, thr, split_thr, max_out, ob.data_ptr(), os_.data_ptr(), ol.data_ptr(),
                                      osrc.data_ptr(), oc.data_ptr(), ws.data_ptr(), nbytes, L.stream_ptr()), "wd_views_merge")

    def value(o):
        want = R.merge(c["boxes"], c["scores"], c["labels"], c["counts"], c["view_flip"], c["img_wh"], n_cls, 0.5, split_thr, max_out,
                       witness=False)
        assert int(want["count"].max()) >= 1
        assert np.array_equal(o["out_count"].cpu().numpy().reshape(-1), want["count"])
        assert np.array_equal(o["out_src"].cpu().numpy(), want["src"])
        assert np.array_equal(o["out_labels"].cpu().numpy(), want["labels"])
        assert np.array_equal(o["out_scores"].cpu().numpy().view(np.uint32), want["scores"].view(np.uint32))
        assert np.array_equal(o["out_boxes"].cpu().numpy().view(np.uint32).reshape(B, max_out, 4), want["boxes"].view(np.uint32))
    return X.Run(launch, lambda: {"out_boxes": ob, "out_scores": os_, "out_labels": ol, "out_src": osrc, "out_count": oc}, value,
                 f"{V} views x {B} images x {max_in} rows, workspace {nbytes} bytes")


@pytest.mark.parametrize("c", CASES, ids=[c.id for c in CASES])
def test_views_extents(c):
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
