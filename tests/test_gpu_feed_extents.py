"""Guard-band tests (GPU) of include/wedetect_hip_feed.h, run exactly as tests/test_gpu_extents.py runs the entry points of the
main header (same harness: its Ctx / Run / Case / execute): every operand of ``wd_feed_batch_u8`` is carved from a
tests/arena.py Arena with guard bands, the case runs in 0x00 and in 0xFF surroundings (outputs bit-identical), inputs stay
unchanged, the tmp arena starts as 0xFF bytes (and as zeros: same bits; a second launch on the dirty tmp: same bits), and the
canvas — which starts out holding the pattern — equals the oracle in every byte, so every byte was written.

The bytes BETWEEN the images of the source arena (each image starts at a multiple of 256) hold the arena's pattern too: they
are outside every documented extent, and differ between the two runs.

tests/test_cpu_feed.py asserts on the CPU that every function of the feed header that takes device memory has a case here.
"""
from __future__ import annotations

from typing import List

import numpy as np
import pytest
import torch

import tests.test_gpu_extents as X
from tests.test_cpu_feed import batch_plans, oracle_canvas, ragged_batch

pytestmark = pytest.mark.gpu

u8, i32 = torch.uint8, torch.int32

CASES: List[X.Case] = []

EXEMPT = {
    "wd_feed_abi_version": "no memory",
    "wd_feed_sizeof_image": "no memory",
    "wd_feed_tmp_bytes": "size query, no memory",
}


def case(entry: str, name: str, cap: int = 64 << 20, **kw):
    def deco(fn):
        CASES.append(X.Case(entry, name, (lambda ctx, _fn=fn, _kw=kw: _fn(ctx, **_kw)), cap))
        return fn
    return deco


def _small_batch(seed):
    """Images for a canvas whose rows are no multiple of 4 bytes or pixels (the byte-store path)."""
    rng = np.random.default_rng(seed)
    img = lambda h, w: rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
    return [(img(21, 31), "cv", 21, 31, "area"), (img(42, 62), "cv", 21, 31, "area"), (img(33, 47), "cv", 20, 31, "area"),
            (img(9, 7), "cv", 23, 31, "bilinear"), (img(375, 500), "pil", 34, 45, None), (img(17, 5), "pil", 50, 15, None),
            (img(9, 601), "pil", 1, 45, None)]


@case("wd_feed_batch_u8", "every mode, 96x128 canvas (dword stores), channels swapped on every other image", which="ragged", canvas=(96, 128), swap=True)
@case("wd_feed_batch_u8", "every mode, 50x45 canvas at an odd address (byte stores, row tail of one pixel)", which="small", canvas=(50, 45), swap=False, dst_mis=1)
@case("wd_feed_batch_u8", "one Pillow image, 64x96 canvas", which="one", canvas=(64, 96), swap=False)
@case("wd_feed_batch_u8", "no Pillow image: no tmp, one launch", which="cv", canvas=(96, 128), swap=True)
def _feed(ctx, which, canvas, swap, dst_mis=4):
    from wedetect_amd import feed as F
    batch = {"ragged": lambda: ragged_batch(3, canvas), "small": lambda: _small_batch(5), "one": lambda: _small_batch(7)[4:5],
             "cv": lambda: ragged_batch(9, canvas)[:5]}[which]()
    plans = batch_plans(batch, canvas, swap)
    offs, nbytes = F.src_offsets([a.shape[:2] for a, *_ in batch])
    src = np.full(nbytes, ctx.ar.pattern, np.uint8)       # the gaps between images look like the surroundings
    for (a, *_), o in zip(batch, offs):
        src[o:o + a.size] = a.reshape(-1)
    packed = F.pack_batch(plans, offs)
    b = len(batch)
    images_host = packed["images"].copy()
    sd = ctx.inp("src", torch.from_numpy(src), mis=1)
    dd = ctx.inp("images", torch.from_numpy(images_host.view(np.uint8).reshape(-1).copy()), mis=8)
    td = ctx.inp("tables", torch.from_numpy(packed["tables"].copy()), mis=4) if packed["table_elems"] else None
    tmp = ctx.ws("tmp", packed["tmp_bytes"], mis=16, row_pitch=F.tmp_bytes(1, max(p["new_w"] for p in plans))) if packed["tmp_bytes"] else None
    dst = ctx.out("dst", (b * canvas[0], canvas[1] * 3), u8, mis=dst_mis)
    launches = F.launches(images_host)
    assert launches == (2 if tmp is not None else 1) <= 3

    def launch():
        ctx.L.check(F.LIB.wd_feed_batch_u8(sd.data_ptr(), nbytes, dd.data_ptr(), images_host.ctypes.data, b,
                                           0 if td is None else td.data_ptr(), packed["table_elems"],
                                           0 if tmp is None else tmp.data_ptr(), packed["tmp_bytes"], dst.data_ptr(),
                                           canvas[0], canvas[1], ctx.L.stream_ptr()), "wd_feed_batch_u8")

    def value(o):
        want = oracle_canvas(batch, plans, canvas)
        got = o["dst"].cpu().numpy().reshape(b, canvas[0], canvas[1], 3)
        for k in range(b):
            assert np.array_equal(got[k], want[k]), f"image {k} (mode {plans[k]['mode']}): {int((got[k] != want[k]).sum())} bytes differ"
    return X.Run(launch, lambda: {"dst": dst}, value,
                 f"{b} images, modes {sorted(set(p['mode'] for p in plans))}, {packed['n_tables']} tables, {launches} launch(es)")


@pytest.mark.parametrize("c", CASES, ids=[c.id for c in CASES])
def test_feed_extents(c):
    run0, o0, f0 = X.execute(c, 0x00, 0xFF)
    run1, o1, f1 = X.execute(c, 0xFF, 0xFF)
    X._same(o0, o1, "surroundings 0x00 vs 0xFF")
    if run0.has_ws:
        _, o2, _ = X.execute(c, 0x00, 0x00)
        X._same(o0, o2, "tmp 0xFF vs zero-filled")
    run0.value(o0)
    print(f"{c.id}: {run0.info}: guards clean, 0x00 == 0xFF" + (", tmp hygiene ok" if run0.has_ws else ""))


def test_feed_refuses_descriptors_outside_their_arenas():
    """The argument checks that keep a bad descriptor from reaching a kernel: nothing is launched, WD_ERR_BAD_ARG."""
    from wedetect_amd import feed as F
    from wedetect_amd import lib as L
    canvas = (96, 128)
    batch = ragged_batch(3, canvas)
    plans = batch_plans(batch, canvas)
    offs, nbytes = F.src_offsets([a.shape[:2] for a, *_ in batch])
    packed = F.pack_batch(plans, offs)
    dev = torch.device("cuda")
    pixels = np.zeros(nbytes, np.uint8)
    for (a, *_), o in zip(batch, offs):
        pixels[o:o + a.size] = a.reshape(-1)
    src = torch.from_numpy(pixels).to(dev)
    ctl = torch.from_numpy(packed["block"].copy()).to(dev)
    tmp = torch.empty(packed["tmp_bytes"], dtype=u8, device=dev)
    dst = torch.full((len(batch), *canvas, 3), 7, dtype=u8, device=dev)

    def call(images, src_bytes=nbytes, elems=packed["table_elems"], tmp_bytes=packed["tmp_bytes"], h=canvas[0], w=canvas[1]):
        return F.LIB.wd_feed_batch_u8(src.data_ptr(), src_bytes, ctl.data_ptr(), images.ctypes.data, len(images),
                                      ctl.data_ptr() + packed["tab_off"], elems, tmp.data_ptr(), tmp_bytes, dst.data_ptr(), h, w,
                                      L.stream_ptr())
    good = packed["images"]
    bad = []
    for field, k, v in (("src_off", 10, nbytes), ("new_w", 0, 129), ("top", 5, 1), ("mode", 2, 9), ("xa", 3, -1),
                        ("yidx", 4, packed["table_elems"]), ("tmp_off", 6, packed["tmp_bytes"]), ("p0", 1, 3), ("fill", 0, -1),
                        ("ksize_v", 7, 0), ("sh", 8, 0)):
        d = good.copy()
        d[field][k] = v
        bad.append((field, call(d)))
    end = max(o + a.size for (a, *_), o in zip(batch, offs))   # nbytes is rounded up to 256: the last image ends before it
    bad += [("src_bytes", call(good, src_bytes=end - 1)), ("table_elems", call(good, elems=packed["table_elems"] - 1)),
            ("tmp_bytes", call(good, tmp_bytes=packed["tmp_bytes"] - 256)), ("dst_h", call(good, h=95))]
    torch.cuda.synchronize()
    assert all(rc == -1 for _, rc in bad), bad
    assert bool((dst == 7).all())                          # nothing ran
    assert call(good) == 0
    torch.cuda.synchronize()
    assert np.array_equal(dst.cpu().numpy(), oracle_canvas(batch, plans, canvas))
