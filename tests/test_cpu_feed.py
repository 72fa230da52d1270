"""The streamed loader without a GPU: the feed header and its binding, the coverage rule of the extent tests applied to the new
header, the host packing of a ragged batch (a numpy interpreter of the descriptor / table format against the oracles), the
scheduler on a stub backend, the entry scripts' new flags and the decode pool's size."""
import ctypes
import fnmatch
import hashlib
import importlib.util
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from tests.abi_decl import declared  # noqa: E402

FEED_HEADER = "wedetect_hip_feed.h"
# sha256 of include/wedetect_hip.h at ABI 15: the feed lives in a header of its own, the frozen one does not move
MAIN_HEADER_SHA256 = "2b62a824664907f02d66fef8abe43f4c50fa0703c00814e15a08129143937784"


# ------------------------------------------------------------------------------------------ library and header
def test_library_exports_the_feed_header_and_the_frozen_abi_is_untouched():
    from wedetect_amd import build as wb
    wb.build(verbose=False)
    decl = set(declared(FEED_HEADER))
    assert {"wd_feed_abi_version", "wd_feed_sizeof_image", "wd_feed_batch_u8", "wd_feed_tmp_bytes"} <= decl
    lib = ctypes.CDLL(wb.LIB)
    missing = [s for s in sorted(decl) if not hasattr(lib, s)]
    assert not missing, f"declared in include/wedetect_hip_feed.h but not exported: {missing}"
    from wedetect_amd import feed as F
    from wedetect_amd import lib as L
    assert set(F.EXPORTS) == decl
    assert not set(F.EXPORTS) & set(L.EXPORTS)
    assert F.LIB.wd_feed_abi_version() == F.FEED_ABI_VERSION
    assert F.LIB.wd_feed_sizeof_image() == ctypes.sizeof(F.FeedImage) == F.IMAGE_DTYPE.itemsize == 96
    for f, _ in F.FeedImage._fields_:                      # the numpy view of a descriptor is the C struct
        assert F.IMAGE_DTYPE.fields[f][1] == getattr(F.FeedImage, f).offset, f
    assert L.LIB.wd_abi_version() == L.ABI_VERSION == 15
    assert hashlib.sha256(open(os.path.join(ROOT, "include", "wedetect_hip.h"), "rb").read()).hexdigest() == MAIN_HEADER_SHA256
    assert "feed.hip" in wb.SOURCES and set(wb.NO_SCRATCH["feed.hip"]) == {"feed_resample_h_kernel", "feed_canvas_kernel"}
    # tmp rows: whole 4-pixel groups at a 16-byte pitch, the image's range rounded to 256
    assert F.tmp_bytes(10, 7) == 512 and F.tmp_bytes(1, 1) == 256 and F.tmp_bytes(480, 640) == 480 * 1920
    assert F.tmp_bytes(3, 5) == 256 and F.tmp_bytes(100, 5) == 100 * 32 + 256 - (100 * 32) % 256


def test_every_feed_entry_point_with_device_memory_has_an_extents_case():
    from tests.test_cpu_arena import EXEMPT_ALLOWED, _takes_memory
    from tests.test_gpu_feed_extents import CASES, EXEMPT
    decl = declared(FEED_HEADER)
    covered = {c.entry for c in CASES}
    allowed = EXEMPT_ALLOWED + ("wd_feed_abi_version", "wd_feed_sizeof_*")
    for name in sorted(decl):
        assert name in covered or name in EXEMPT, f"{name}: feed entry without a case in tests/test_gpu_feed_extents.py (or an EXEMPT reason)"
        assert not (name in covered and name in EXEMPT), f"{name}: both covered and exempt"
    for name, reason in EXEMPT.items():
        assert name in decl, f"EXEMPT names {name}, which the header does not declare"
        assert isinstance(reason, str) and reason.strip() and "\n" not in reason
        assert any(fnmatch.fnmatch(name, pat) for pat in allowed), f"{name} may not be exempt: it must have a case"
        assert not _takes_memory(decl[name]), f"{name} takes device memory: it must have a case"
    assert _takes_memory(decl["wd_feed_batch_u8"]) and "wd_feed_batch_u8" in covered
    assert not covered - set(decl)
    ids = [c.id for c in CASES]
    assert len(ids) == len(set(ids)), "case ids must be unique"


# ------------------------------------------------------------------------------------------ packing
PREC = 22


def _clip8(v):
    return np.clip(v >> PREC, 0, 255).astype(np.uint8)


def _cv_round(v):                                          # float32 -> int, half to even, saturated to uint8
    return np.clip(np.rint(v.astype(np.float32)), 0, 255).astype(np.uint8)


def interpret(block: np.ndarray, n_img: int, tab_off: int, src: np.ndarray, canvas_hw):
    """What wd_feed_batch_u8 computes, read from the packed control block alone: descriptors at 0, tables at ``tab_off``."""
    from wedetect_amd import feed as F
    images = block[: n_img * F.IMAGE_DTYPE.itemsize].view(F.IMAGE_DTYPE)
    ti = block[tab_off:].view(np.int32)
    tf = block[tab_off:].view(np.float32)
    H, W = canvas_hw
    out = np.zeros((n_img, H, W, 3), np.uint8)
    for b in range(n_img):
        d = images[b]
        sh, sw, nh, nw, top, left, mode = (int(d[k]) for k in ("sh", "sw", "new_h", "new_w", "top", "left", "mode"))
        off = int(d["src_off"])
        assert off % 256 == 0
        s = src[off:off + sh * sw * 3].reshape(sh, sw, 3).astype(np.int64)
        fill = int(d["fill"])
        out[b] = np.array([fill & 255, (fill >> 8) & 255, (fill >> 16) & 255], np.uint8)
        xa, xidx, xw, ya, yidx, yw = (int(d[k]) for k in F.TABLE_FIELDS)
        if mode == 0:
            assert (nh, nw) == (sh, sw)
            r = s.astype(np.uint8)
        elif mode == 1:
            isx, isy = int(d["p0"]), int(d["p1"])
            box = s[:nh * isy, :nw * isx].reshape(nh, isy, nw, isx, 3).sum(axis=(1, 3))
            r = ((box + 2) >> 2).astype(np.uint8) if (isx, isy) == (2, 2) else _cv_round(box.astype(np.float32) * np.float32(d["p2"]))
        elif mode == 2:
            r = np.zeros((nh, nw, 3), np.uint8)
            xr, yr = ti[xa:xa + 2 * nw].reshape(nw, 2), ti[ya:ya + 2 * nh].reshape(nh, 2)
            sf = s.astype(np.float32)
            # horizontal sums per source row, in tap order, multiply and add rounded separately (float32)
            hbuf = np.zeros((sh, nw, 3), np.float32)
            for dx in range(nw):
                xs, xn = xr[dx]
                acc = np.zeros((sh, 3), np.float32)
                for k in range(xn):
                    acc = acc + sf[:, ti[xidx + xs + k]] * tf[xw + xs + k]
                hbuf[:, dx] = acc
            for dy in range(nh):
                ys, yn = yr[dy]
                acc = None
                for j in range(yn):
                    term = tf[yw + ys + j] * hbuf[ti[yidx + ys + j]]
                    acc = term if acc is None else acc + term
                r[dy] = _cv_round(acc)
        elif mode == 3:
            xc, yc = ti[xa:xa + 2 * nw].reshape(nw, 2).astype(np.int64), ti[ya:ya + 2 * nh].reshape(nh, 2).astype(np.int64)
            sx = ti[xidx:xidx + nw].astype(np.int64)
            sy0 = np.clip(ti[yidx:yidx + nh].astype(np.int64), 0, sh - 1)
            sy1 = np.clip(ti[yidx:yidx + nh].astype(np.int64) + 1, 0, sh - 1)
            two = np.arange(nw) < int(d["p0"])
            sx1 = np.where(two, sx + 1, sx)
            assert sx1.max() < sw

            def hpass(rows):
                a = s[rows][:, sx] * xc[None, :, 0, None] + s[rows][:, sx1] * xc[None, :, 1, None]
                return np.where(two[None, :, None], a, s[rows][:, sx] * 2048)
            h0, h1 = hpass(sy0), hpass(sy1)
            r = ((((yc[:, 0, None, None] * (h0 >> 4)) >> 16) + ((yc[:, 1, None, None] * (h1 >> 4)) >> 16) + 2) >> 2).astype(np.uint8)
        else:
            assert mode == F.FEED_PILLOW
            ksh, ksv = int(d["ksize_h"]), int(d["ksize_v"])
            bh, bv = ti[xa:xa + 2 * nw].reshape(nw, 2), ti[ya:ya + 2 * nh].reshape(nh, 2)
            kh = ti[xidx:xidx + nw * ksh].reshape(nw, ksh).astype(np.int64)
            kv = ti[yidx:yidx + nh * ksv].reshape(nh, ksv).astype(np.int64)
            tmp = np.zeros((sh, nw, 3), np.int64)
            for xx in range(nw):
                x0, n = bh[xx]
                tmp[:, xx] = _clip8((1 << (PREC - 1)) + (s[:, x0:x0 + n] * kh[xx, :n, None]).sum(axis=1))
            r = np.zeros((nh, nw, 3), np.uint8)
            for yy in range(nh):
                y0, n = bv[yy]
                r[yy] = _clip8((1 << (PREC - 1)) + (tmp[y0:y0 + n] * kv[yy, :n, None, None]).sum(axis=0))
        if int(d["swap_rb"]):
            r = r[..., ::-1]
        out[b, top:top + nh, left:left + nw] = r
    return out


def ragged_batch(seed=0, canvas=(96, 128)):
    """[(image, kind, new_h, new_w, interp)]: every mode of the feed once, and a 1-pixel-wide image."""
    rng = np.random.default_rng(seed)
    img = lambda h, w: rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
    return [
        (img(40, 60), "cv", 40, 60, "area"),               # COPY
        (img(80, 120), "cv", 40, 60, "area"),              # AREA_FAST 2 x 2
        (img(90, 150), "cv", 30, 50, "area"),              # AREA_FAST 3 x 3
        (img(75, 101), "cv", 45, 61, "area"),              # general AREA
        (img(20, 31), "cv", 50, 77, "bilinear"),           # LINEAR
        (img(200, 150), "pil", 96, 72, None),              # Pillow shrink
        (img(17, 23), "pil", 95, 128, None),               # Pillow enlarge
        (img(64, 1), "pil", 96, 2, None),                  # 1 pixel wide, Pillow
        (img(33, 1), "cv", 90, 3, "bilinear"),             # 1 pixel wide, LINEAR
        (img(80, 120), "cv", 40, 60, "area"),              # the tables / geometry of image 1 again
        (img(75, 101), "cv", 45, 61, "area"),              # shares all six tables with image 3
    ]


def batch_plans(batch, canvas, swap=False):
    from wedetect_amd import feed as F
    H, W = canvas
    plans = []
    for k, (a, kind, nh, nw, interp) in enumerate(batch):
        top, left = (H - nh) // 2, (W - nw) // 2
        sw_ = bool(swap) and k % 2 == 0
        if kind == "cv":
            plans.append(F.plan_cv(a.shape[0], a.shape[1], nh, nw, interp, top, left, 114, swap_rb=sw_))
        else:
            plans.append(F.plan_pillow(a.shape[0], a.shape[1], nh, nw, top, left, (114, 113, 112), swap_rb=sw_))
    return plans


def oracle_canvas(batch, plans, canvas):
    from oracle import cv2_resize as cv
    from oracle import resample
    H, W = canvas
    out = np.zeros((len(batch), H, W, 3), np.uint8)
    for b, ((a, kind, nh, nw, interp), p) in enumerate(zip(batch, plans)):
        if kind == "cv":
            r = a if (nh, nw) == a.shape[:2] else cv.cv2_resize_u8(a, (nw, nh), interp)
            out[b] = 114
        else:
            r = resample.resize_bilinear_u8(a, nw, nh)
            out[b] = np.array([114, 113, 112], np.uint8)
        out[b, p["top"]:p["top"] + nh, p["left"]:p["left"] + nw] = r[..., ::-1] if p["swap_rb"] else r
    return out


@pytest.mark.parametrize("swap", [False, True])
def test_packed_batch_reproduces_the_oracles(swap):
    from wedetect_amd import feed as F
    from wedetect_amd import lib as L
    canvas = (96, 128)
    batch = ragged_batch()
    plans = batch_plans(batch, canvas, swap)
    modes = [p["mode"] for p in plans]
    assert modes[:9] == [L.CVRESIZE_COPY, L.CVRESIZE_AREA_FAST, L.CVRESIZE_AREA_FAST, L.CVRESIZE_AREA, L.CVRESIZE_LINEAR,
                         F.FEED_PILLOW, F.FEED_PILLOW, F.FEED_PILLOW, L.CVRESIZE_LINEAR]
    assert (plans[1]["p0"], plans[1]["p1"]) == (2, 2) and (plans[2]["p0"], plans[2]["p1"]) == (3, 3)
    offs, nbytes = F.src_offsets([a.shape[:2] for a, *_ in batch])
    assert all(o % 256 == 0 for o in offs) and nbytes % 256 == 0
    src = np.full(nbytes, 0xA5, np.uint8)                  # what lies between the images is never read
    for (a, *_), o in zip(batch, offs):
        src[o:o + a.size] = a.reshape(-1)
    packed = F.pack_batch(plans, offs)
    total, tab_off, elems = F.control_bytes(plans)
    assert packed["block"].size == total and packed["tab_off"] == tab_off and tab_off % 256 == 0 and packed["table_elems"] == elems
    # dedup: the second 2 x 2 image has no tables, the second AREA image points at the first one's six
    im = packed["images"]
    for f in F.TABLE_FIELDS:
        assert im[f][10] == im[f][3] >= 0
        assert im[f][0] == im[f][1] == im[f][2] == -1
    distinct = {key for p in plans for key, _ in p["tables"].values()}
    assert packed["n_tables"] == len(distinct) < sum(len(p["tables"]) for p in plans)
    assert elems == sum(arr.size for key, arr in {k: a for p in plans for k, a in p["tables"].values()}.items())
    # tmp ranges: Pillow images only, disjoint, 256-aligned
    pil = [k for k, p in enumerate(plans) if p["mode"] == F.FEED_PILLOW]
    ranges = sorted((int(im["tmp_off"][k]), int(im["tmp_off"][k]) + plans[k]["tmp_bytes"]) for k in pil)
    assert all(a % 256 == 0 for a, _ in ranges) and all(r0[1] <= r1[0] for r0, r1 in zip(ranges, ranges[1:]))
    assert packed["tmp_bytes"] >= ranges[-1][1]
    assert F.launches(im) == 2 and F.launches(im[:5]) == 1
    got = interpret(packed["block"], len(batch), tab_off, src, canvas)
    want = oracle_canvas(batch, plans, canvas)
    for b in range(len(batch)):
        assert np.array_equal(got[b], want[b]), f"image {b} (mode {modes[b]}): {int((got[b] != want[b]).sum())} bytes differ"
    # packing into a caller's (pinned) block writes the same bytes
    mine = np.full(total + 100, 7, np.uint8)
    again = F.pack_batch(plans, offs, mine)
    assert np.array_equal(again["images"], im) and np.array_equal(again["tables"], packed["tables"]) and (mine[total:] == 7).all()
    with pytest.raises(ValueError):
        F.pack_batch(plans, offs, np.zeros(total - 1, np.uint8))


# ------------------------------------------------------------------------------------------ scheduler on a stub
class StubBackend:
    """Records what the scheduler asks for; results are ("r", item)."""

    def __init__(self, trip_on=None, fallback_batches=0):
        self.slot = [None, None]
        self.state = [None, None]                          # None / "uploaded" / "issued"
        self.log, self.in_flight, self.max_in_flight = [], 0, 0
        self.trip_on, self.fallback_batches, self.fallback = trip_on, fallback_batches, 0
        self.decoding = [0, 0]

    def decode(self, item, slot):
        if isinstance(item, str) and item.startswith("missing"):
            raise FileNotFoundError(item)
        return dict(h=1, w=1)

    def input_free(self, slot):
        self.log.append(("free", slot))

    def upload(self, slot, items, geoms):
        assert self.state[slot] != "issued", "upload over a batch that is still in flight"
        assert len(items) == len(geoms)
        self.slot[slot], self.state[slot] = list(items), "uploaded"
        self.log.append(("upload", tuple(items)))

    def issue(self, slot):
        assert self.state[slot] == "uploaded"
        self.state[slot] = "issued"
        self.in_flight += 1
        self.max_in_flight = max(self.max_in_flight, self.in_flight)
        self.log.append(("issue", tuple(self.slot[slot])))

    def collect(self, slot):
        assert self.state[slot] == "issued"
        self.state[slot] = "uploaded"
        self.in_flight -= 1
        items = self.slot[slot]
        self.log.append(("collect", tuple(items)))
        if self.trip_on is not None and self.trip_on in items:
            self.trip_on = None
            self.fallback = self.fallback_batches
            return True, []
        return False, [("r", it) for it in items]

    def inline(self, slot):
        assert self.state[slot] == "uploaded" and self.in_flight == 0, "in-line step beside steps in flight"
        self.log.append(("inline", tuple(self.slot[slot])))
        self.fallback = max(0, self.fallback - 1)
        return [("r", it) for it in self.slot[slot]]

    def inline_only(self):
        return self.fallback > 0

    def drain(self):
        for k in (0, 1):
            if self.state[k] == "issued":
                self.state[k] = "uploaded"
        self.in_flight = 0
        self.log.append(("drain",))


@pytest.mark.parametrize("n,bs", [(0, 4), (1, 4), (4, 4), (7, 4), (8, 4), (9, 4), (26, 4), (5, 1), (3, 32)])
def test_scheduler_order_depth_and_tail(n, bs):
    from wedetect_amd.stream import StreamScheduler
    be = StubBackend()
    sch = StreamScheduler(be, bs, decode_workers=3)
    out = list(sch.run(list(range(n))))
    assert out == [("r", k) for k in range(n)]             # input order, each exactly once
    assert be.max_in_flight <= 2 and sch.stats["max_in_flight"] == be.max_in_flight
    assert sch.stats["batches"] == -(-n // bs) and sch.stats["trips"] == 0
    issues = [e for e in be.log if e[0] == "issue"]
    assert len(issues) == -(-n // bs)
    if n >= 3 * bs:                                        # steady state: step i is issued before step i - 1 is read
        order = [e for e in be.log if e[0] in ("issue", "collect")]
        assert order.index(("issue", tuple(range(bs, 2 * bs)))) < order.index(("collect", tuple(range(bs))))
        assert be.max_in_flight == 2
    if n % bs and n > bs:                                  # a tail of another size drains first
        tail = tuple(range(n - n % bs, n))
        at = be.log.index(("issue", tail))
        assert all(e in be.log[:at] for e in [("collect", tuple(range(k, k + bs))) for k in range(0, n - n % bs, bs)])
    assert (be.log == []) if n == 0 else (be.log[-1] == ("drain",))


def test_scheduler_decode_failure_names_the_path():
    from wedetect_amd.stream import DecodeError, StreamScheduler
    be = StubBackend()
    items = ["a.jpg", "b.jpg", "c.jpg", "d.jpg", "e.jpg", "missing/f.jpg", "g.jpg"]
    got = []
    with pytest.raises(DecodeError, match="missing/f.jpg"):
        for r in StreamScheduler(be, 2).run(items):
            got.append(r)
    assert got == [("r", it) for it in items[:len(got)]] and len(got) <= 4
    assert be.log[-1] == ("drain",)                        # nothing is left in flight


class _PathBackend(StubBackend):
    def decode(self, item, slot):
        if isinstance(item, dict):
            raise OSError("truncated file")
        return super().decode(item, slot)


def test_scheduler_decode_failure_names_a_data_info():
    from wedetect_amd.stream import DecodeError, StreamScheduler
    with pytest.raises(DecodeError, match="/data/x.jpg.*truncated"):
        list(StreamScheduler(_PathBackend(), 2).run([dict(img_path="/data/x.jpg", img_id=3)]))


@pytest.mark.parametrize("trip_item,fallback", [(5, 0), (5, 2), (0, 0), (13, 0), (9, 1)])
def test_scheduler_trip_reruns_in_line_and_reissues(trip_item, fallback):
    from wedetect_amd.stream import StreamScheduler
    n, bs = 14, 4
    be = StubBackend(trip_on=trip_item, fallback_batches=fallback + 1 if fallback else 0)
    sch = StreamScheduler(be, bs)
    out = list(sch.run(list(range(n))))
    assert out == [("r", k) for k in range(n)]             # each image once, in order
    assert be.max_in_flight <= 2 and sch.stats["trips"] == 1
    j = trip_item // bs
    batch = lambda k: tuple(range(k * bs, min(n, (k + 1) * bs)))
    at = be.log.index(("collect", batch(j)))
    assert be.log[at + 1] == ("drain",) and be.log[at + 2] == ("inline", batch(j))
    nxt = j + 1
    if nxt * bs < n and len(batch(nxt)) == bs:             # it had been issued beside the tripped one: issued or run again
        before = [e for e in be.log[:at] if e == ("issue", batch(nxt))]
        after = [e for e in be.log[at:] if e in (("issue", batch(nxt)), ("inline", batch(nxt)))]
        assert len(before) == 1 and len(after) == 1
        assert after[0][0] == ("inline" if fallback else "issue")
        assert sch.stats["reissued"] == 1
    inlined = [e for e in be.log if e[0] == "inline"]
    assert len(inlined) == 1 + min(fallback, -(-n // bs) - 1 - j) and sch.stats["inline_batches"] == len(inlined)
    assert sch.stats["batches"] == -(-n // bs)


# ------------------------------------------------------------------------------------------ parsers
def test_entry_scripts_take_the_loader_flags():
    spec = importlib.util.spec_from_file_location("wd_test_entry_feed", os.path.join(ROOT, "test.py"))
    T = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(T)
    a = T.parse_args(["cfg.py", "ckpt.pth", "--loader", "stream", "--decode-workers", "4"])
    assert a.loader == "stream" and a.decode_workers == 4
    a = T.parse_args(["cfg.py", "ckpt.pth"])
    assert a.loader == "serial" and a.decode_workers is None
    with pytest.raises(SystemExit):
        T.parse_args(["cfg.py", "ckpt.pth", "--loader", "dataloader"])
    for flag in (["--tta"], ["--show"], ["--show-dir", "x"]):
        with pytest.raises(SystemExit):
            T.parse_args(["cfg.py", "ckpt.pth", "--loader", "stream", *flag])
    spec = importlib.util.spec_from_file_location("wd_eval_recall_feed", os.path.join(ROOT, "eval_recall", "eval_recall.py"))
    E = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(E)
    a = E.parse_args(["--dataset", "coco", "--loader", "stream", "--decode-workers", "4"])
    assert a.loader == "stream" and a.decode_workers == 4
    assert E.parse_args([]).loader == "serial"


def test_stream_pipeline_shape_is_checked_by_name():
    from wedetect_amd.cfgfile import Config
    from wedetect_amd.stream import check_stream_pipeline
    cfg = Config.fromfile(os.path.join(ROOT, "config", "wedetect_tiny.py"))
    pipe = cfg.test_dataloader.dataset.pipeline
    pipe = [p.to_dict() if hasattr(p, "to_dict") else dict(p) for p in pipe]
    assert [type(t).__name__ for t in check_stream_pipeline(pipe)] == ["LoadImageFromFile", "WeDetectKeepRatioResize",
                                                                      "WeDetectLetterResize", "LoadAnnotations", "LoadText", "PackDetInputs"]
    with pytest.raises(NotImplementedError, match="LoadAnnotations"):
        check_stream_pipeline(pipe[:2] + pipe[3:])
    with pytest.raises(NotImplementedError, match="PackDetInputs"):
        check_stream_pipeline(pipe[:-1])


# ------------------------------------------------------------------------------------------ decode pool
def test_decode_pool_ignores_the_cpu_count(monkeypatch):
    from wedetect_amd import stream as S
    monkeypatch.setattr(os, "cpu_count", lambda: 512)
    monkeypatch.delenv("OMP_NUM_THREADS", raising=False)
    assert S.decode_pool_size() == 8
    for env, want in (("16", 12), ("4", 4), ("512", 12), ("", 8), ("x", 8)):
        monkeypatch.setenv("OMP_NUM_THREADS", env)
        assert S.decode_pool_size() == want
    assert S.decode_pool_size(3) == 3 and S.decode_pool_size(400) == 12
    with pytest.raises(ValueError):
        S.decode_pool_size(0)
    assert S.StreamScheduler(StubBackend(), 4).workers <= 12
    src = open(os.path.join(ROOT, "wedetect_amd", "stream.py")).read()
    assert "cpu_count" not in src
